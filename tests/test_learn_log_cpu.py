"""CPU: the learn log (include/ttenv.h: tt_learn_log_*, csrc/ttlearnlog.hip) without a GPU -- the kernel's resources read from the
library's code object, what the five entry points refuse before any HIP call, the job struct's layout, and the Python refusals."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from ddpg_trucktrailer_amd import _lib
    return _lib


def test_one_kernel_without_scratch_or_spills_at_two_waves_per_simd(L):
    from ddpg_trucktrailer_amd import kernel_resources as kr
    found = kr.find(kr.kernels(), "k_learn_log")
    assert len(found) == 1, sorted(found)
    (name, v), = found.items()
    assert v["scratch"] == 0 and v["vgpr_spills"] == 0, (name, v)
    assert kr.waves_per_simd(v["vgpr"]) >= 2, (name, v)
    assert v["max_threads"] == 256 and 2 * v["lds"] <= 160 * 1024, (name, v)
    # the names the resource tests of the existing kernels search by must not find it
    for part in ("k_step", "k_fwd_multi", "k_fwd_small", "k_bwd_rows_pair", "k_bwd_weights", "k_actor_tail", "k_mlp_split",
                 "k_pop_fwd_multi"):
        assert part not in name, (part, name)


def _job(L, **kw):
    j = L.TTLearnLogJob()
    for n in ("y", "q", "q_pi", "dq_da", "mu", "grad_critic", "grad_actor", "step_dev"):
        setattr(j, n, 0x1000)            # (never dereferenced: every call here is refused before any HIP call)
    j.numel_critic, j.numel_actor = 132201, 131601
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def test_entry_points_refuse_bad_arguments_by_name(L):
    dll = L.load()
    assert dll.tt_version() == 3
    msg = lambda: dll.tt_last_error(None).decode()
    h = C.c_void_p()
    jobs = (L.TTLearnLogJob * 1)(_job(L))

    def create(agents=1, batch=256, jobs=jobs, capacity=4, every=1, out=C.byref(h)):
        return dll.tt_learn_log_create(agents, batch, jobs, capacity, every, out)
    for kw, word in ((dict(out=None), "out"), (dict(jobs=None), "jobs"), (dict(agents=0), "agents"),
                     (dict(agents=L.POP_MAX_AGENTS + 1), "agents"), (dict(batch=0), "batch"), (dict(batch=1025), "batch"),
                     (dict(capacity=0), "capacity"), (dict(capacity=L.LEARN_LOG_MAX_CAPACITY + 1), "capacity"), (dict(every=0), "every"),
                     (dict(jobs=(L.TTLearnLogJob * 1)(_job(L, numel_critic=0))), "numel"),
                     (dict(jobs=(L.TTLearnLogJob * 1)(_job(L, numel_actor=-3))), "numel"),
                     (dict(jobs=(L.TTLearnLogJob * 1)(_job(L, grad_actor=0x1004))), "aligned")) + tuple(
                         (dict(jobs=(L.TTLearnLogJob * 1)(_job(L, **{n: None}))), "NULL")
                         for n in ("y", "q", "q_pi", "dq_da", "mu", "grad_critic", "grad_actor", "step_dev")):
        h.value = 0x5555
        assert create(**kw) == L.TT_EINVAL, kw
        assert "tt_learn_log_create" in msg() and word in msg(), (kw, msg())
        assert "out" in kw or h.value is None, kw                  # (no handle comes back from a refusal)
    n = C.c_int64(7)
    assert dll.tt_learn_log_append(None, None) == L.TT_EINVAL and "tt_learn_log_append" in msg()
    assert dll.tt_learn_log_clear(None, None) == L.TT_EINVAL and "tt_learn_log_clear" in msg()
    assert dll.tt_learn_log_destroy(None) == L.TT_EINVAL and "tt_learn_log_destroy" in msg()
    assert dll.tt_learn_log_drain(None, 0, -1, 0, None, None, None, C.byref(n)) == L.TT_EINVAL and "tt_learn_log_drain" in msg()
    assert dll.tt_learn_log_drain(C.c_void_p(0x1000), 0, -1, 0, None, None, None, None) == L.TT_EINVAL and "count" in msg()


def test_job_struct_and_constants_follow_the_header(L):
    src = open(os.path.join(ROOT, "include", "ttenv.h")).read()
    body = re.search(r"typedef struct tt_learn_log_job \{(.*?)\} tt_learn_log_job;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size, names = 0, []
    for decl in (d.strip() for d in body.split(";") if d.strip()):
        pointer = "*" in decl
        width = 8 if pointer else {"int32_t": 4, "int64_t": 8, "float": 4}[decl.split()[0]]
        for name in decl.split(",") if pointer else decl.split(None, 1)[1].split(","):
            size = (size + width - 1) // width * width + width
            names.append(name.split("*")[-1].strip())
    size = (size + 7) // 8 * 8
    assert size == 72 and C.sizeof(L.TTLearnLogJob) == size
    assert names == [n for n, _ in L.TTLearnLogJob._fields_]
    defines = dict(re.findall(r"#define (TT_LEARN_LOG_\w+) (.+)", src))
    assert int(defines["TT_LEARN_LOG_NVALUES"]) == len(L.LEARN_LOG_VALUES) == 16
    assert int(defines["TT_LEARN_LOG_CHUNKS"]) == L.LEARN_LOG_CHUNKS
    assert eval(defines["TT_LEARN_LOG_MAX_CAPACITY"]) == L.LEARN_LOG_MAX_CAPACITY
    for name in L.LEARN_LOG_VALUES:                                # the header's table names every value
        assert re.search(rf"\b{name}\b", src), name


class _Env:
    """What DDPGRollout's constructor asks of an env (tests/test_nstep.py's stand-in)."""
    n_envs, observation_dim = 8, 23

    def __init__(self):
        import torch
        self.device = torch.device("cpu")

    def observe(self, out):
        out.zero_()


def test_python_side_refuses_a_learn_log_without_the_fused_learner_on_a_gpu(L):
    from ddpg_trucktrailer_amd.population import PopulationRollout
    from ddpg_trucktrailer_amd.rollout import DDPGRollout
    with pytest.raises(ValueError, match="learn_log"):
        DDPGRollout(_Env(), replay_slots=16, batch_size=4, learn_log=8)
    with pytest.raises(ValueError, match="learn_log"):
        DDPGRollout(_Env(), replay_slots=16, batch_size=4, learn_log=8, fused_learn=False)
    with pytest.raises(ValueError, match="learn_log"):
        PopulationRollout(64, [1, 2], device="cpu", learn_log=8)
    for kw in (dict(learn_log=8, learn_log_every=0), dict(learn_log=0)):
        with pytest.raises(ValueError, match="learn_log"):
            DDPGRollout(_Env(), replay_slots=16, batch_size=4, **kw)
        with pytest.raises(ValueError, match="learn_log"):
            PopulationRollout(64, [1, 2], device="cpu", **kw)
    loop = DDPGRollout(_Env(), replay_slots=16, batch_size=4)      # off: nothing changes, and a drain says so
    with pytest.raises(ValueError, match="learn log is off"):
        loop.drain_learn_log()
