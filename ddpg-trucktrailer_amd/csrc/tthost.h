// tthost.h -- what the library's host code shares across its sources: the one way to refuse a call (format a message, return a
// code) and the refusals every n-step entry point makes.  Host only (no device code, no HIP call); defined once in csrc/ttenv.hip.
#pragma once

#include <cstdarg>

namespace tthost {

constexpr int ERR_BYTES = 256;      // every message buffer: the library's, a tt_env's, a tt_p2p's

// formats the message into dst[ERR_BYTES] and returns `code`: the helper under every refusal, whichever buffer it writes
int vfail(char *dst, int code, const char *fmt, va_list ap) __attribute__((format(printf, 3, 0)));

// sets the library's message (tt_last_error(NULL)) and returns `code`
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

// What an n-step draw refuses whoever makes it, in the two places its callers check them: n_step outside 1 .. TT_NSTEP_MAX or
// gamma outside (0, 1); and a ring of `slots` slots that, with its `reserve` newest slots kept out, has no base step with all
// its n steps in the window.  TT_OK, or TT_EINVAL with the message "<who>: <reason>".
int refuse_nstep(const char *who, int n_step, float gamma);
int refuse_nstep_window(const char *who, int n_step, int slots, int reserve);

}  // namespace tthost
