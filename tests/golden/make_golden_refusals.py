"""Writes tests/golden/refusals.json: bad calls that libttenv.so refuses before any HIP call, each with the return code and the
message (tt_last_error(NULL)) it leaves.  Run once against the library whose messages are to be pinned:

    TT_LIB_PATH=/path/to/that/libttenv.so python tests/golden/make_golden_refusals.py

tests/test_refusals_cpu.py replays the table (its docstring has the argument notation) against the library of the tree.  No GPU is
needed: no call of the table reaches a HIP call, and no pointer of the table is dereferenced."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

P = {"ptr": 0x1000}                    # a non-NULL pointer or handle that the refused call never follows
S, A, S2 = {"ptr": 0x2000}, {"ptr": 0x3000}, {"ptr": 0x4000}      # the draw's s, a and s' buffers
N = None


def sample(**kw):
    f = dict(batch=4, n_envs=2, slots=8, reserve=0, k_dev=P, obs=P, act=P, rew=P, done=P, seed=1, s_out=S, a_out=A, r_out=P,
             s2_out=S2, d_out=P, lag=0, draws=1)
    f.update(kw)
    return {"struct": "TTSampleArgs", "fields": f}


def side(count):
    return {"struct": "TTSideBuffer", "fields": dict(obs=P, act=P, rew=P, obs2=P, done=P, count=count)}


def jobs(*items):
    return {"array": "TTFwdJob", "items": list(items)}


def agents(*items):
    return {"array": "TTPopAgent", "items": list(items)}


def pairs(*items):
    return {"array": "TTPopExploitPair", "items": [dict(zip(("dst", "src", "alpha", "beta", "tau", "gamma"), p)) for p in items]}


def log_job(**kw):
    f = dict(y=P, q=P, q_pi=P, dq_da=P, mu=P, grad_critic=P, grad_actor=P, step_dev=P, numel_critic=132201, numel_actor=131601)
    f.update(kw)
    return {"array": "TTLearnLogJob", "items": [f]}


H = {"out": "ptr"}
CASES = [
    # (every tt_env entry point with a NULL handle and nothing else comes first: main() makes those calls from _lib._SIGNATURES)
    ("tt_env_set_episode_log", [N, -1, N]), ("tt_env_rollout_random", [N, -1, 0, N, N, N, N]),
    # unknown flag bits are refused before the handle is looked at
    ("tt_env_set_episode_log2", [N, 0, 1, N]), ("tt_env_set_episode_log2", [N, 0, 2, N]), ("tt_env_set_episode_log2", [N, 0, 7, N]),
    ("tt_env_set_episode_log2", [N, -1, 0xFFFFFFFE, N]),
    # ---- the handle-less entry points of the same source
    ("tt_params_default", [2, N]), ("tt_params_default", [0, N]), ("tt_env_create", [4, 0, N, N]), ("tt_env_create", [0, 0, N, H]),
    ("tt_env_create", [-5, 0, N, H]), ("tt_random_actions", [-1, 0, 0, N, N]), ("tt_random_actions", [5, 0, 0, N, N]),
    # ---- the n-step draw: no sample, n_step, gamma, the sample itself, the window, a side buffer, draws -- in this order
    ("tt_ring_sample_nstep", [N, 0, 2.0, N]), ("tt_ring_sample_nstep", [sample(n_envs=0), 0, 2.0, N]),
    ("tt_ring_sample_nstep", [sample(n_envs=0), 17, 0.5, N]), ("tt_ring_sample_nstep", [sample(n_envs=0), 16, 1.0, N]),
    ("tt_ring_sample_nstep", [sample(n_envs=0), 1, 0.0, N]), ("tt_ring_sample_nstep", [sample(n_envs=0, slots=3), 4, 0.5, N]),
    ("tt_ring_sample_nstep", [sample(slots=2), 1, 0.5, N]), ("tt_ring_sample_nstep", [sample(obs=N), 1, 0.5, N]),
    ("tt_ring_sample_nstep", [sample(slots=5, side=side(3), draws=2), 4, 0.5, N]),
    ("tt_ring_sample_nstep", [sample(slots=9, reserve=4), 4, 0.5, N]),
    ("tt_ring_sample_nstep", [sample(side=side(3), draws=2), 2, 0.5, N]), ("tt_ring_sample_nstep", [sample(side=side(3), draws=2), 1, 0.5, N]),
    ("tt_ring_sample_nstep", [sample(draws=7), 3, 0.5, N]),
    # ---- learn()'s first launch with that draw: its own arguments first, then the draw's refusals under its name, then the jobs
    ("tt_mlp_forward_multi_sampled_nstep", [-1, 4, P, N, 0, 2.0, N, N]), ("tt_mlp_forward_multi_sampled_nstep", [4, 0, P, N, 0, 2.0, N, N]),
    ("tt_mlp_forward_multi_sampled_nstep", [4, 5, P, N, 0, 2.0, N, N]), ("tt_mlp_forward_multi_sampled_nstep", [4, 4, N, N, 0, 2.0, N, N]),
    ("tt_mlp_forward_multi_sampled_nstep", [4, 4, P, N, 0, 2.0, N, N]), ("tt_mlp_forward_multi_sampled_nstep", [4, 4, P, sample(batch=5), 0, 2.0, N, N]),
    ("tt_mlp_forward_multi_sampled_nstep", [4, 4, P, sample(batch=5), 2, 2.0, N, N]),
    ("tt_mlp_forward_multi_sampled_nstep", [4, 4, P, sample(batch=-1), 2, 0.5, N, N]),
    ("tt_mlp_forward_multi_sampled_nstep", [4, 4, P, sample(batch=5, slots=4), 3, 0.5, N, N]),
    ("tt_mlp_forward_multi_sampled_nstep", [4, 4, P, sample(batch=5, side=side(2)), 3, 0.5, N, N]),
    ("tt_mlp_forward_multi_sampled_nstep", [4, 4, P, sample(batch=5, draws=3), 3, 0.5, N, N]),
    ("tt_mlp_forward_multi_sampled_nstep", [4, 4, P, sample(batch=5), 3, 0.5, N, N]),
    ("tt_mlp_forward_multi_sampled_nstep", [4, 1, jobs({}), sample(), 3, 0.5, N, N]),
    ("tt_mlp_forward_multi_sampled_nstep", [4, 2, jobs({}, {}), sample(), 1, 0.5, N, N]),
    # ---- populations
    ("tt_pop_learn_create", [0, 0, N, N]), ("tt_pop_learn_create", [0, 0, N, H]), ("tt_pop_learn_create", [17, 0, N, H]),
    ("tt_pop_learn_create", [16, 0, N, H]), ("tt_pop_learn_create", [1, 1025, N, H]), ("tt_pop_learn_create", [1, 1024, N, H]),
    ("tt_pop_learn_create", [1, 256, agents({}), H]), ("tt_pop_learn_create", [2, 256, agents(dict(sample=sample(batch=256)), {}), H]),
    ("tt_pop_learn_create", [1, 256, agents(dict(sample=sample(batch=64, draws=2))), H]),
    ("tt_pop_learn_create", [1, 256, agents(dict(sample=sample(batch=256, draws=2, side=side(1), obs=N))), H]),
    ("tt_pop_learn_create", [1, 256, agents(dict(sample=sample(batch=256, step_progress=P))), H]),
    ("tt_pop_learn_create", [1, 256, agents(dict(sample=sample(batch=256, side=side(1), obs=N))), H]),
    ("tt_pop_learn_create", [1, 256, agents(dict(sample=sample(batch=256, obs=N))), H]),
    ("tt_pop_learn_create", [1, 256, agents(dict(sample=sample(batch=256))), H]),
    ("tt_pop_learn_create", [1, 256, agents(dict(sample=sample(batch=256), jobs=jobs({}, {}, {}, {}))), H]),
    ("tt_pop_learn", [N, -1, N]), ("tt_pop_learn", [N, 0, N]),
    ("tt_pop_exploit", [N, 0, N, N]), ("tt_pop_exploit", [P, 0, N, N]), ("tt_pop_exploit", [N, 1, pairs((0, 1, .1, .1, .1, .9)), N]),
    ("tt_pop_exploit_nstep", [N, 0, N, N, N]), ("tt_pop_exploit_nstep", [P, 0, N, N, N]),
    ("tt_pop_exploit_nstep", [N, 1, pairs((0, 1, .1, .1, .1, .9)), N, N]),
    ("tt_pop_learn_set_nstep", [N, N]), ("tt_pop_learn_set_nstep", [P, N]), ("tt_pop_learn_set_nstep", [N, {"out": "nstep"}]),
    ("tt_pop_nstep", [N, 0, N]), ("tt_pop_nstep", [P, 0, N]), ("tt_pop_nstep", [N, -1, {"out": "nstep"}]),
    ("tt_pop_hyper", [N, 0, N]), ("tt_pop_hyper", [P, 0, N]), ("tt_pop_hyper", [N, -1, {"out": "f32x4"}]),
    # ---- the learn log
    ("tt_learn_log_create", [0, 0, N, 0, 0, N]), ("tt_learn_log_create", [0, 0, N, 0, 0, H]), ("tt_learn_log_create", [17, 0, N, 0, 0, H]),
    ("tt_learn_log_create", [1, 0, N, 0, 0, H]), ("tt_learn_log_create", [1, 1025, N, 0, 0, H]), ("tt_learn_log_create", [1, 256, N, 0, 0, H]),
    ("tt_learn_log_create", [1, 256, log_job(), 0, 0, H]), ("tt_learn_log_create", [1, 256, log_job(), (1 << 22) + 1, 0, H]),
    ("tt_learn_log_create", [1, 256, log_job(), 1 << 40, 0, H]), ("tt_learn_log_create", [1, 256, log_job(), -(1 << 40), 0, H]),
    ("tt_learn_log_create", [1, 256, log_job(), 4, 0, H]), ("tt_learn_log_create", [1, 256, log_job(y=N, numel_critic=0), 4, -2, H]),
    ("tt_learn_log_create", [1, 256, log_job(step_dev=N, numel_critic=0), 4, 1, H]),
    ("tt_learn_log_create", [1, 256, log_job(numel_critic=0, grad_actor={"ptr": 0x1004}), 4, 1, H]),
    ("tt_learn_log_create", [1, 256, log_job(numel_actor=-3, grad_actor={"ptr": 0x1004}), 4, 1, H]),
    ("tt_learn_log_create", [1, 256, log_job(grad_actor={"ptr": 0x1004}), 4, 1, H]),
    ("tt_learn_log_create", [1, 256, log_job(grad_critic={"ptr": 0x1008}), 4, 1, H]),
    ("tt_learn_log_append", [N, N]), ("tt_learn_log_clear", [N, N]), ("tt_learn_log_destroy", [N]),
    ("tt_learn_log_drain", [N, 0, -1, 0, N, N, N, N]), ("tt_learn_log_drain", [N, 0, -1, 0, N, N, N, {"out": "i64"}]),
    ("tt_learn_log_drain", [P, 0, -1, 0, N, N, N, N]),
]


def main():
    from ddpg_trucktrailer_amd import _lib as L
    from test_refusals_cpu import TABLE, call
    table = []
    quiet = ("tt_env_destroy", "tt_env_num_envs", "tt_env_state_bytes", "tt_env_episode_log_bytes")      # (these leave no message)
    null_handle = [(fn, [N if t is L._P or hasattr(t, "contents") else 0 for t in argtypes])
                   for fn, (_, argtypes) in L._SIGNATURES.items() if fn.startswith("tt_env_") and fn != "tt_env_create" and fn not in quiet]
    for fn, args in null_handle + CASES:
        case = {"fn": fn, "args": args}
        case["code"], case["message"] = call(L, case)
        assert case["code"] != L.TT_OK and case["message"].startswith(fn), case      # a refusal, and this call's own message
        table.append(case)
    with open(TABLE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in table) + "\n]\n")
    print(f"{TABLE}: {len(table)} refusals of {len({c['fn'] for c in table})} entry points from {L.LIB_PATH}")


if __name__ == "__main__":
    main()
