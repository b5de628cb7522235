// tthost.h -- what the library's host code shares across its sources: the message of tt_last_error(NULL) and the refusals every
// n-step entry point makes.  Host only (no device code, no HIP call); defined once in csrc/ttenv.hip.
#pragma once

namespace tthost {

// sets the library's message (tt_last_error(NULL)) and returns `code`
int fail_library(int code, const char *msg);

// TT_EINVAL with the message `fmt`, formatted with up to two ints
int einval(const char *fmt, int a = 0, int b = 0);

// What an n-step draw refuses whoever makes it, in the two places its callers check them: n_step outside 1 .. TT_NSTEP_MAX or
// gamma outside (0, 1); and a ring of `slots` slots that, with its `reserve` newest slots kept out, has no base step with all
// its n steps in the window.  TT_OK, or TT_EINVAL with the message "<who>: <reason>".
int refuse_nstep(const char *who, int n_step, float gamma);
int refuse_nstep_window(const char *who, int n_step, int slots, int reserve);

}  // namespace tthost
