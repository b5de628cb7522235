"""CPU: the plain and the shaped entry points of learn()'s rows, weight and tail launches go through one checked conversion each
(csrc/ttlearn_host.h), on made-up addresses: what both refuse they refuse in the same words, each under its own name; and where the
shaped launch refuses what the plain one takes, the plain call gets past every host check up to the conversion's last."""
import pytest

import fake_args as F


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib as L
    return L


def _refusal(L, form, entry, spoils):
    f = F.Fake(L, 256, form)
    for spoil in spoils:
        spoil(f)
    rc = getattr(f, entry)()
    return rc, f.last_error()


# every spoiled argument of the shaped entry points' tables that the plain entry point refuses as well: all but the critic flag of the
# weight launch, which the plain launch takes (below)
_BOTH = [(e, w, s) for e, rs in (("rows", F.ROWS), ("weights", F.WEIGHTS), ("tail_", F.TAIL)) for w, s in rs if (e, w) != ("weights", "critic")]


@pytest.mark.parametrize("entry, word, spoil", _BOTH, ids=[f"{e}-{i}-{w.replace(' ', '_')}" for i, (e, w, _) in enumerate(_BOTH)])
def test_the_plain_entry_point_refuses_in_its_shaped_twins_words_under_its_own_name(lib, entry, word, spoil):
    """TT_EINVAL from both, and the plain call's message is the shaped call's with the function's name substituted."""
    rc_s, msg_s = _refusal(lib, "shaped", entry, [spoil])
    rc_p, msg_p = _refusal(lib, "plain", entry, [spoil])
    shaped, plain = F.entry_name(entry, "shaped"), F.entry_name(entry, "plain")
    assert rc_s == lib.TT_EINVAL and msg_s.startswith(shaped + ":") and word in msg_s, (rc_s, msg_s)
    assert rc_p == lib.TT_EINVAL, (rc_p, msg_p)
    assert msg_p == plain + msg_s[len(shaped):], (msg_p, msg_s)


def _as_critic(f):
    f.critic_flag, f.action, f.count = 1, f.nxt(), 12


def _no_row_factors(f):
    f.dq_da = f.mu = None


# What the shaped weight launch refuses and the plain one takes.  No call here may launch (the addresses are made up), so each case
# also loses the step count, which the conversion checks last of all (to_weights_launch: the optimizer step): the plain call's
# message names that and nothing before it, the shaped call's names the difference.  (count = 0 -- gradients only -- is taken by
# both launches and skips that last check: past it there is only the launch, so it is not shown here.)
_TAKEN = [("critic", [_as_critic], "critic"),
          ("no row factors", [_no_row_factors], "row_dq_da or row_mu"),
          ("n = 1025 without factors", [_no_row_factors, lambda f: setattr(f, "B", 1025)], "row_dq_da or row_mu")]


@pytest.mark.parametrize("name, spoils, word", _TAKEN, ids=[t[0].replace(" ", "_") for t in _TAKEN])
def test_what_only_the_shaped_weight_launch_refuses_passes_the_plain_ones_host_checks(lib, name, spoils, word):
    no_step = lambda f: setattr(f, "step", None)
    rc_s, msg_s = _refusal(lib, "shaped", "weights", spoils + [no_step])
    assert rc_s == lib.TT_EINVAL and msg_s.startswith("tt_mlp_backward_weights_shaped:") and word in msg_s, (rc_s, msg_s)
    rc_p, msg_p = _refusal(lib, "plain", "weights", spoils + [no_step])
    assert rc_p == lib.TT_EINVAL and msg_p == "tt_mlp_backward_weights: the optimizer step lacks a tensor or the step count", (rc_p, msg_p)
    # with row factors the plain launch is bound to n <= 1024 as well: the table above holds that case
    assert ("weights", "n = 1025") in [(e, w) for e, w, _ in _BOTH]
