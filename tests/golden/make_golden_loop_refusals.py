"""Writes tests/golden/loop_refusals.json: calls of the loops' options -- the six option values, the check_* functions, the option
blocks of the loops and learners, the checkpoint refusals -- each with its outcome (tests/test_loop_refusals_cpu.py has the
notation).  Run once against the commit whose behaviour is to be pinned, with that commit's package first on the path and this
tree's tests/ for the replay code -- a `git worktree` of the commit will do:

    git worktree add --detach /tmp/parent <commit>
    TT_PACKAGE_ROOT=/tmp/parent python tests/golden/make_golden_loop_refusals.py <commit>

The table was written from 25c7afa, the commit before the options moved onto ddpg_trucktrailer_amd/options.py.  No GPU is needed:
every call ends, or is refused, on the host."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.environ.get("TT_PACKAGE_ROOT", ROOT), os.path.dirname(HERE)]

NAN, INF, ENV = {"float": "nan"}, {"float": "inf"}, {"cpu_env": True}
FORCE_DP = {"TT_FORCE_DP": "1"}


def new(name, *args, set=None, **kw):
    return dict({"new": name, "args": list(args), "kwargs": kw}, **({"set": set} if set else {}))


def case(call, *args, environ=None, method=None, margs=None, set=None, **kw):
    c = {"call": call, "args": list(args), "kwargs": kw}
    for k, v in (("env", environ), ("method", method), ("margs", margs), ("set", set)):
        if v is not None:
            c[k] = v
    return c


def many(call, *variants, **common):
    """One case per variant (a dict of keyword arguments, or a tuple of positional ones) on top of the common keywords."""
    return [case(call, *v, **common) if isinstance(v, tuple) else case(call, **dict(common, **v)) for v in variants]


def td3(*a, **k): return new("td3.TD3Config", *a, **k)
def shape(*a, **k): return new("loss_shape.LossShape", *a, **k)
def demo(*a, **k): return new("demo_loss.DemoLoss", *a, **k)
def mpc(*a, **k): return new("mpc.MPCConfig", *a, **k)
def lanes(*a, **k): return new("mpc.ExpertLanes", *a, **k)
def labels(*a, **k): return new("mpc.ExpertLabels", *a, **k)
def agent(**k): return new("agent.Agent", 1e-4, 1e-3, {"tuple": [23]}, 1e-3, 1, fc1_dims=8, fc2_dims=8, device="cpu", replay=False, **k)
def ring(slots=8): return new("replay_buffer.TrajectoryRing", 4, slots, 23, "cpu")
def ns(**k): return new("types.SimpleNamespace", **k)
def sd(**k): return {"dict": dict({"batch_size": 4}, **k)}


def the(name): return {"the": name}
def zeros(*shape, **k): return new("torch.zeros", list(shape), **k)


LEARNER = dict(agent=ns(td3=None), grad_sync_critic=None, p2p=None, B=4, dev=new("torch.device", "cpu"), loss_shape=None, demo_loss=None,
               labels=None, learn_log=None)
BATCH = [zeros(4, 23), zeros(4, 1), zeros(4), zeros(4, 23), zeros(4, dtype=the("torch.uint8"))]
INDEX = zeros(4, 2, dtype=the("torch.int32"))


def bare(method, *margs, **attrs):
    """A case on a FusedLearner made without its constructor: LEARNER's attributes, then attrs, then the method."""
    return {"bare": "fused_learn.FusedLearner", "set": dict(LEARNER, **attrs), "method": method, "margs": list(margs)}


SMALL = mpc(horizon=5, samples=65)
MPC_T = [5, 65, 0.3, 0.8, 10.0, 1.0, 20.0, 300.0]
LOOP = dict(batch_size=4, replay_slots=8, fc1_dims=8, fc2_dims=8, use_graph=False)
STEPPER = dict(batch_size=4, replay_slots=8, fc1_dims=8, fc2_dims=8)

CASES = (
    # ---- TD3Config: policy_delay, then target_noise, then noise_clip.  True is a number to it, and a string or None never reaches its message
    many("td3.TD3Config", dict(policy_delay=0), dict(policy_delay=True), dict(policy_delay=2.5), dict(policy_delay=-1),
         dict(policy_delay="a"), dict(policy_delay=None), dict(policy_delay=0, target_noise=-1), dict(target_noise=-0.1),
         dict(target_noise=NAN), dict(noise_clip=INF), dict(target_noise="0.2"), dict(noise_clip=None),
         dict(target_noise=-1, noise_clip=-1), (), (2.0, 1, 0), dict(target_noise=True), dict(noise_clip=False), (4, 0.1, 0.3))
    # ---- LossShape: huber_delta, then pre_penalty
    + many("loss_shape.LossShape", dict(huber_delta=0), dict(huber_delta=-1.0), dict(huber_delta=True), dict(huber_delta="1"),
           dict(huber_delta=NAN), dict(huber_delta=INF), dict(pre_penalty=-1), dict(pre_penalty=True), dict(pre_penalty=NAN),
           dict(pre_penalty=None), dict(huber_delta=0, pre_penalty=-1), (), (2, 1), (None, 0), (0.5, 2.0))
    # ---- DemoLoss: bc_weight, then q_filter
    + many("demo_loss.DemoLoss", (0,), (-1.0,), (True,), (NAN,), ("1",), (None,), (1, 2), (1, "yes"), (1, None), (1, 1.0), (0, 2),
           (1,), (2.0, 0), (0.5, 1), (1, False))
    # ---- MPCConfig / check_mpc: the fields in their order, then the action scale, then the buffers
    + many("mpc.MPCConfig", dict(horizon=0), dict(horizon=65), dict(horizon=2.0), dict(horizon=True), dict(samples=0),
           dict(samples=1025), dict(samples="8"), dict(sigma=-1), dict(sigma=NAN), dict(sigma=True), dict(k_lat=-1), dict(k_yaw=INF),
           dict(rho=1), dict(rho=-0.1), dict(rho=NAN), dict(temperature=0), dict(temperature=INF), dict(gamma=0), dict(gamma=1.5),
           dict(horizon=0, samples=0), dict(samples=0, sigma=-1), dict(k_yaw=-1, rho=2), dict(rho=2, temperature=0),
           dict(temperature=0, gamma=0), (), (1, 1, 0, 0, 1, 1, 0, 0), dict(horizon=64, samples=1024, rho=0.999, gamma=0.5))
    + many("mpc.check_mpc", dict(action_scale=0), dict(action_scale=NAN), dict(action_scale=True),
           dict(action_scale=0.785), dict(n_envs=4), dict(n_envs=4, plan="x", mu_out="y"),
           dict(n_envs=4, plan=new("torch.zeros", [4, 40]), mu_out="y"),
           dict(n_envs=4, plan=new("torch.zeros", [4, 39]), mu_out=new("torch.zeros", 4)),
           dict(n_envs=4, plan=new("torch.zeros", [4, 40]), mu_out=new("torch.zeros", 4), live=new("torch.zeros", 4)),
           dict(n_envs=4, plan=new("torch.zeros", [4, 40]), mu_out=new("torch.zeros", 4), returns_out=new("torch.zeros", [4, 256])),
           dict(n_envs=4, plan=new("torch.zeros", [4, 40]), mu_out=new("torch.zeros", 4)), cfg=mpc())
    + many("mpc.check_mpc", (3,), (None,), (SMALL,), (mpc(set={"horizon": 65, "samples": 0}),))
    # ---- ExpertLanes / check_expert_lanes
    + many("mpc.ExpertLanes", (0,), (-2,), (2.0,), (True,), ("3",), (None,), (2, "mpc"), (2, {"tuple": [5, 65]}), dict(lanes=2, seed=-1),
           dict(lanes=2, seed=2 ** 64), dict(lanes=2, seed=1.5), dict(lanes=2, seed=True), dict(lanes=0, seed=-1), dict(lanes=0, mpc="mpc"),
           (1,), (3, SMALL, 7), dict(lanes=2, seed=2 ** 64 - 1))
    + many("mpc.check_expert_lanes", (3,), ({"tuple": [3, None, 0]},), (labels(2),), (lanes(2, mpc(set={"horizon": 65})),),
           (lanes(2, set={"lanes": 0, "seed": -1}),), (lanes(2, set={"mpc": 5}),), (lanes(3),))
    + many("mpc.check_expert_lanes", dict(n_envs=2), dict(n_envs=3), dict(ring_mode=False), dict(ring_mode=True), dict(population=True),
           dict(data_parallel=True), dict(force_dp=True), dict(n_envs=2, ring_mode=False), dict(ring_mode=False, population=True),
           dict(population=True, data_parallel=True), dict(data_parallel=True, force_dp=True), expert=lanes(3))
    # ---- ExpertLabels / check_expert_labels
    + many("mpc.ExpertLabels", (0,), (2.0,), (True,), (2, {"tuple": [5, 65]}), dict(lanes=2, seed=2 ** 64), dict(lanes=2, seed=-1),
           dict(lanes=0, seed=-1), dict(lanes=0, mpc=3), (2,), (3, SMALL, 7))
    + many("mpc.check_expert_labels", (3,), (lanes(2),), (labels(2, mpc(set={"samples": 0})),), (labels(2, set={"lanes": 0, "seed": -1}),),
           (labels(2),))
    + many("mpc.check_expert_labels", dict(expert=2), dict(expert=lanes(2, set={"lanes": 0})), dict(expert=lanes(2, SMALL)),
           dict(expert=lanes(2, seed=3)), dict(expert=lanes(2, SMALL, seed=3)), dict(expert=lanes(2, seed=3), n_envs=4),
           dict(expert=lanes(2), n_envs=4), dict(expert=lanes(2), n_envs=5), dict(n_envs=2), dict(n_envs=3), dict(ring_mode=False),
           dict(population=True), dict(data_parallel=True), dict(force_dp=True), dict(demo_loss=None), dict(demo_loss=demo(1)),
           dict(n_envs=2, ring_mode=False), dict(ring_mode=False, population=True), dict(population=True, data_parallel=True),
           dict(data_parallel=True, force_dp=True), dict(force_dp=True, demo_loss=None), labels=labels(3))
    # ---- the four other check_* functions and check_learn_log
    + many("loss_shape.check_loss_shape", (3,), (None,), (demo(1),), (shape(),))
    + many("loss_shape.check_loss_shape", dict(td3=td3()), dict(population=True), dict(data_parallel=True), dict(force_dp=True),
           dict(td3=td3(), population=True), dict(population=True, data_parallel=True), dict(data_parallel=True, force_dp=True),
           shape=shape(2, 0.5))
    + many("demo_loss.check_demo_loss", (3,), (shape(),), (demo(1),))
    + many("demo_loss.check_demo_loss", dict(td3=td3()), dict(population=True), dict(data_parallel=True), dict(force_dp=True),
           dict(n_step=3), dict(n_step=3.0), dict(n_step=1), dict(td3=td3(), population=True), dict(population=True, data_parallel=True),
           dict(data_parallel=True, force_dp=True), dict(force_dp=True, n_step=2), demo=demo(1))
    + many("td3.check_td3", (3,), (None,), (td3(),), (td3(), 2), (td3(), 3), (td3(3), 2), (td3(), 2, 2), (td3(), 2, 1, True),
           (td3(), 2, 1, False, True), (td3(), 2, 1, False, None, 16), (td3(), 3, 2), (td3(), 2, 2, True), (td3(), 2, 1, True, True),
           (td3(), 2, 1, False, True, 16), (td3(1),))
    + many("td3.check_population_td3", (td3(), 2, 2), ([td3(), td3(2, 0.1)], 2, 2), ([td3()], 2, 2), ([td3(), 3], 2, 2), (3, 2, 2),
           ([td3(), 3, 4], 2, 2), ([td3(), td3(3)], 2, 6), ([td3(), td3(3)], 2, 1), (td3(), 2, 3), (td3(), 2, 3, [1, 2]),
           (td3(), 2, 2, [1, 2]), (td3(), 2, 2, [1, 2], 2), (td3(), 2, 2, [1], 2), (td3(), 2, 2, [1], 2, 16), (td3(), 2, 2, [1], 1, 16),
           (td3(), 2, 2, [1], 1, 16, "cpu"), (td3(), 2, 2, [1], 1, None, "cpu"), (td3(), 2, 3, [1], 1, None, "no such device"),
           (td3(), 2, 2, [1, 2], 1, None, "no such device"), (td3(), 2, 2, [1], 2, 16, "no such device"),
           (td3(), 2, 2, [1], 1, 16, "no such device"))
    + many("fused_learn.check_learn_log", (0,), (2 ** 40,), (16, 0), (0, 0), (16, 2), (16,), (1.0, 1.0))
    # ---- DDPGRollout: each option's refusals through the loop, on a CPU device
    + many("rollout.DDPGRollout", dict(labels=labels(2)), dict(labels=2, demo_loss=demo(1)), dict(labels=labels(5), demo_loss=demo(1)),
           dict(labels=labels(3), expert=lanes(2), demo_loss=demo(1)), dict(labels=labels(2), expert=lanes(2, seed=3), demo_loss=demo(1)),
           dict(labels=labels(2), demo_loss=demo(1)), dict(labels=labels(2), demo_loss=demo(1), data_parallel=True),
           dict(labels=labels(2), demo_loss=demo(1), world_size=2), dict(labels=labels(2), demo_loss=demo(1), dp_exchange="p2p"),
           dict(expert=2), dict(expert=lanes(5)), dict(expert=lanes(2)), dict(expert=lanes(2), data_parallel=True),
           dict(expert=lanes(2), world_size=2), dict(expert=lanes(2), dp_exchange="p2p"), dict(expert=lanes(2), data_parallel=False, world_size=2),
           dict(n_step=0), dict(n_step=17), dict(n_step=None), dict(n_step=None, demo_loss=3), dict(demo_loss=3), dict(demo_loss=demo(1), td3=td3()), dict(demo_loss=demo(1), n_step=3),
           dict(demo_loss=demo(1), data_parallel=True), dict(demo_loss=demo(1), world_size=2), dict(demo_loss=demo(1), dp_exchange="p2p"),
           dict(loss_shape=3), dict(loss_shape=shape(), td3=td3()), dict(loss_shape=shape(), data_parallel=True),
           dict(loss_shape=shape(), dp_exchange="p2p"), dict(td3=3), dict(td3=td3()), dict(td3=td3(), updates_per_step=2, n_step=2),
           dict(td3=td3(), updates_per_step=2, data_parallel=True), dict(td3=td3(), updates_per_step=2, dp_exchange="p2p"),
           dict(td3=td3(), updates_per_step=2, pipeline=True), dict(td3=td3(), updates_per_step=2, learn_log=16), dict(learn_log=0),
           dict(learn_log=16, learn_log_every=0), dict(learn_log=16), dict(n_step=3, replay_slots=4), dict(n_step=2, data_parallel=True),
           dict(n_step=2, world_size=2), dict(data_parallel=True), dict(dp_exchange="p2p", data_parallel=True),
           # two bad options: each adjacent pair of labels, expert, n_step, demo_loss, loss_shape, td3, learn_log, replay_slots, ranks
           dict(labels=2, expert=2), dict(expert=2, n_step=0), dict(n_step=0, demo_loss=3), dict(demo_loss=3, loss_shape=3),
           dict(loss_shape=3, td3=3), dict(td3=3, learn_log=0), dict(learn_log=0, n_step=3, replay_slots=4),
           dict(n_step=3, replay_slots=4, data_parallel=True), dict(labels=labels(2), expert=2), dict(labels=2, td3=3),
           # what is accepted
           dict(), dict(td3=td3(), updates_per_step=2), dict(loss_shape=shape(2, 0.5), demo_loss=demo(3)), dict(n_step=2),
           dict(td3=td3(), updates_per_step=2, pipeline=False), env=ENV, **LOOP)
    + many("rollout.DDPGRollout", dict(labels=labels(2), demo_loss=demo(1)), dict(expert=lanes(2)), dict(demo_loss=demo(1)),
           dict(loss_shape=shape()), dict(td3=td3(), updates_per_step=2), dict(n_step=2), dict(learn_log=16), dict(),
           dict(expert=lanes(2), demo_loss=demo(1)), dict(demo_loss=demo(1), loss_shape=shape()), environ=FORCE_DP, env=ENV, **LOOP)
    # ---- DDPGRollout: the agent passed in was built with other options than the loop (six texts), and where that sits in the order
    + many("rollout.DDPGRollout", dict(agent=agent(demo_loss=demo(1)), demo_loss=demo(2)), dict(agent=agent(), demo_loss=demo(2)),
           dict(agent=agent(demo_loss=demo(1))), dict(agent=agent(loss_shape=shape(2)), loss_shape=shape(3)),
           dict(agent=agent(), loss_shape=shape(3)), dict(agent=agent(loss_shape=shape(2))), dict(agent=agent(), td3=td3(), updates_per_step=2),
           dict(agent=agent(td3=td3())), dict(agent=agent(demo_loss=demo(1)), loss_shape=3), dict(agent=agent(loss_shape=shape(2)), td3=3),
           dict(agent=agent(td3=td3()), learn_log=0), dict(agent=agent(demo_loss=demo(1), loss_shape=shape(2))),
           dict(agent=agent(demo_loss=demo(1)), n_step=0), dict(agent=agent(td3=td3(4, 0.1)), td3=td3(), updates_per_step=4),
           dict(agent=agent(demo_loss=demo(1), loss_shape=shape(2)), demo_loss=demo(1), loss_shape=shape(2)), env=ENV, **LOOP)
    # ---- VectorStepper: expert and labels, after ring_mode is known
    + many("stepper.VectorStepper", dict(expert=lanes(2)), dict(labels=labels(2)), dict(expert=2), dict(labels=2), dict(expert=lanes(5)),
           dict(labels=labels(5)), dict(expert=lanes(2), labels=labels(3)), dict(expert=2, labels=2), dict(), dict(td3=td3()),
           env=ENV, **STEPPER)
    # ---- PopulationRollout: everything before the first env is made
    + many("population.PopulationRollout", dict(loss_shape=shape()), dict(loss_shape=3), dict(demo_loss=demo(1)), dict(demo_loss=3),
           dict(expert=lanes(2)), dict(expert=3), dict(loss_shape=shape(), demo_loss=demo(1)), dict(demo_loss=demo(1), expert=lanes(2)),
           dict(expert=lanes(2), td3=3), dict(td3=3), dict(td3=td3()), dict(td3=[td3()], updates_per_step=2),
           dict(td3=[td3(), td3(3)], updates_per_step=2), dict(td3=td3(), updates_per_step=2, n_step=2),
           dict(td3=td3(), updates_per_step=2, n_step_max=2), dict(td3=td3(), updates_per_step=2, learn_log=16),
           dict(td3=td3(), updates_per_step=2, device="cpu"), dict(td3=3, learn_log=0), dict(learn_log=0), dict(learn_log=16, learn_log_every=0),
           dict(learn_log=16, device="cpu"), dict(learn_log=0, data_parallel=True), dict(data_parallel=True), dict(pipeline=True),
           dict(side_buffer=3), dict(data_parallel=True, seeds=[]), dict(seeds=[]), dict(seeds=list(range(17))), dict(n_step=[1, 2, 3]),
           dict(n_step=0), dict(n_step=[1, 2], n_step_max=1), dict(n_step=2, device="cpu"), dict(n_step=3, replay_slots=4),
           dict(n_step=1, n_step_max=3, replay_slots=4), dict(alphas=[1e-4]), dict(gammas=[0.9, 0.9, 0.9], alphas=[1e-4]),
           n_envs_per_agent=4, seeds=[1, 2])
    # ---- PopulationLearner: the options, also as attributes of the agents it is given, then its own arguments
    + many("population.PopulationLearner", dict(loss_shape=shape()), dict(demo_loss=demo(1)), dict(expert=lanes(2)), dict(expert=3),
           dict(loss_shape=shape(), demo_loss=demo(1)), dict(demo_loss=demo(1), expert=lanes(2)), dict(agents=[ns(loss_shape=shape())]),
           dict(agents=[ns(), ns(demo_loss=demo(1))]), dict(agents=[ns(demo_loss=demo(1)), ns(loss_shape=shape())]),
           dict(agents=[ns(loss_shape=3)]), dict(agents=[ns(expert=lanes(2))]), dict(agents=[ns(expert=3)]), dict(agents=[ns(loss_shape=shape())], demo_loss=demo(1)), dict(),
           dict(agents=[ns(loss_shape=None, demo_loss=None)]), dict(agents=[ns()], rings=[ring()]), dict(agents=[ns()], rings=[ring(), ring()], seeds=[1]),
           dict(agents=[ns()], rings=[ring(4)], seeds=[1], n_steps=3), dict(agents=[ns()], rings=[ring()], seeds=[1], n_steps=[1, 2]),
           dict(agents=[ns()], rings=[ring()], seeds=[1], n_steps=17), dict(agents=[ns()], rings=[ring()], seeds=[1], learn_log=0),
           dict(agents=[ns()], rings=[ring(4)], seeds=[1], n_steps=3, learn_log=0), agents=[], batch_size=4)
    # ---- FusedLearner: what it refuses before it touches the agent
    + many("fused_learn.FusedLearner", dict(expert_lanes=-1), dict(expert_lanes=True), dict(expert_lanes=2.0), dict(expert_lanes=3),
           dict(labels=[0, 0]), dict(labels=[1]), dict(labels=[1.0, 2]), dict(labels=[0, 2]), dict(labels=[1, 2], demo_loss=demo(1), expert_lanes=2),
           dict(labels=[0, 0], expert_lanes=-1), dict(labels=[0, 2], expert_lanes=3), dict(labels=[-1, 2], demo_loss=demo(1)),
           agent=None, batch_size=4)
    # ---- FusedLearner's setters and checks that raise before they touch the device, on a bare learner
    + [bare("set_loss_shape", 3), bare("set_loss_shape", None), bare("set_loss_shape", demo(1)),
       bare("set_loss_shape", shape(), agent=ns(td3=td3())), bare("set_loss_shape", shape(), grad_sync_critic=1),
       bare("set_loss_shape", shape(), p2p=1), bare("set_loss_shape", 3, agent=ns(td3=td3()), p2p=1),
       bare("set_loss_shape", shape(), agent=ns(td3=td3()), grad_sync_critic=1), bare("set_loss_shape", shape(2, 0.5), agent=ns()),
       bare("set_demo_loss", 3), bare("set_demo_loss", shape()), bare("set_demo_loss", demo(1), agent=ns(td3=td3())),
       bare("set_demo_loss", demo(1), grad_sync_critic=1), bare("set_demo_loss", demo(1), p2p=1),
       bare("set_demo_loss", 3, agent=ns(td3=td3()), grad_sync_critic=1), bare("set_demo_loss", demo(1), agent=ns(td3=td3()), p2p=1),
       bare("set_demo_loss", demo(1), agent=ns()),
       bare("set_label_array", zeros(8, 4)), bare("set_label_array", "x"), bare("set_label_array", "x", labels={"tuple": [1, 2]}),
       bare("set_label_array", new("torch.arange", 8), labels={"tuple": [1, 2]}),
       bare("set_label_array", zeros(8, 4, dtype=the("torch.float64")), labels={"tuple": [1, 2]}),
       bare("set_label_array", zeros(8, 2), labels={"tuple": [1, 2]}), bare("set_label_array", zeros(8, 3), labels={"tuple": [1, 2]}),
       bare("_refuse_ranks_with_loss_shape"), bare("_refuse_ranks_with_loss_shape", loss_shape=shape()),
       bare("_refuse_ranks_with_loss_shape", demo_loss=demo(1)), bare("_refuse_ranks_with_loss_shape", loss_shape=shape(), demo_loss=demo(1)),
       bare("enable_data_parallel", loss_shape=shape()), bare("enable_data_parallel", demo_loss=demo(1)),
       bare("enable_data_parallel", learn_log=1), bare("enable_data_parallel", learn_log=1, loss_shape=shape()),
       bare("enable_p2p", loss_shape=shape()), bare("enable_p2p", demo_loss=demo(1)), bare("enable_p2p", learn_log=1, demo_loss=demo(1)),
       bare("learn_batch", *BATCH, demo_loss=demo(1)), bare("learn_batch", *BATCH, None, None, None, 3, INDEX, demo_loss=demo(1)),
       bare("learn_batch", *BATCH, None, None, None, 1, INDEX),
       bare("demo_stats"), bare("append_learn_log"), bare("drain_learn_log"), bare("enable_learn_log", 16, learn_log=1),
       bare("load_state_dict", {"dict": {"loss_shape": [2.0, 0.5]}}), bare("load_state_dict", {"dict": {"demo_loss": [1.0, True]}}),
       bare("load_state_dict", {"dict": {"loss_shape": [2.0, 0.5], "demo_loss": [1.0, True]}}),
       bare("load_state_dict", {"dict": {"loss_shape": None, "demo_loss": None}}),
       bare("load_state_dict", {"dict": {}}, loss_shape=shape(2, 0.5), demo_loss=demo(3)),
       bare("load_state_dict", {"dict": {"loss_shape": [2.0, 0.5]}}, loss_shape=shape(2, 0.5), demo_loss=demo(3)),
       bare("load_state_dict", {"dict": {"loss_shape": [2.0, 0.25], "demo_loss": [3.0, False]}}, loss_shape=shape(2, 0.5), demo_loss=demo(3)),
       bare("load_state_dict", {"dict": {"loss_shape": [2.0, 0.5], "demo_loss": [3.0, False]}}, loss_shape=shape(2, 0.5), demo_loss=demo(3)),
       bare("load_state_dict", {"dict": {"loss_shape": [2.0, 0.5], "demo_loss": [3.0, True]}}, loss_shape=shape(2, 0.5), demo_loss=demo(3))]
    # ---- checkpoints: each of the five keys in both directions, and pairs for the order
    + many("rollout.DDPGRollout", dict(margs=[sd(n_step=2)]), dict(margs=[sd(batch_size=8)]), dict(margs=[sd(td3=[2, 0.2, 0.5])]),
           dict(margs=[sd(loss_shape=[2.0, 0.5])]), dict(margs=[sd(demo_loss=[1.0, True])]), dict(margs=[sd(expert=[2, MPC_T, 0])]),
           dict(margs=[sd(labels=[2, MPC_T, 0])]), dict(margs=[sd(n_step=2, td3=[2, 0.2, 0.5])]),
           dict(margs=[sd(td3=[2, 0.2, 0.5], loss_shape=[2.0, 0.5])]), dict(margs=[sd(loss_shape=[2.0, 0.5], demo_loss=[1.0, True])]),
           dict(margs=[sd(demo_loss=[1.0, True], expert=[2, MPC_T, 0])]), dict(margs=[sd(expert=[2, MPC_T, 0], labels=[2, MPC_T, 0])]),
           dict(margs=[sd(loss_shape=None, demo_loss=None, expert=None, labels=[1, MPC_T, 3])]), env=ENV, method="load_state_dict", **LOOP)
    + many("rollout.DDPGRollout", dict(margs=[sd()]), dict(margs=[sd(td3=[2, 0.2, 0.5], loss_shape=[None, 0.0])]), env=ENV,
           method="load_state_dict", td3=td3(), updates_per_step=2, **LOOP)
    + many("rollout.DDPGRollout", dict(margs=[sd()]), dict(margs=[sd(loss_shape=[2.0, 0.5])]), dict(margs=[sd(loss_shape=[2.0, 0.25], demo_loss=[3.0, False])]),
           dict(margs=[sd(loss_shape=[2.0, 0.5], demo_loss=[3.0, False])]), dict(margs=[sd(loss_shape=[2.0, 0.5], demo_loss=[3.0, True], expert=[1, MPC_T, 0])]),
           env=ENV, method="load_state_dict", loss_shape=shape(2, 0.5), demo_loss=demo(3), **LOOP)
    + many("stepper.VectorStepper", dict(margs=[{"dict": {}}]), dict(margs=[{"dict": {"expert": [2, MPC_T, 0]}}]),
           dict(margs=[{"dict": {"labels": [2, MPC_T, 0]}}]), dict(margs=[{"dict": {"expert": [2, MPC_T, 0], "labels": [2, MPC_T, 0]}}]),
           dict(margs=[{"dict": {}}], set={"expert": lanes(2, SMALL)}), dict(margs=[{"dict": {}}], set={"labels": labels(2, SMALL)}),
           dict(margs=[{"dict": {}}], set={"expert": lanes(2, SMALL), "labels": labels(2, SMALL)}),
           dict(margs=[{"dict": {"expert": [2, MPC_T, 0]}}], set={"expert": lanes(3, SMALL)}),
           dict(margs=[{"dict": {"expert": [2, MPC_T, 0]}}], set={"expert": lanes(2, SMALL)}),
           dict(margs=[{"dict": {"expert": [2, MPC_T, 0], "labels": [1, MPC_T, 1]}}], set={"expert": lanes(2, SMALL), "labels": labels(1, SMALL)}),
           dict(margs=[{"dict": {"expert": [2, MPC_T, 0], "labels": [1, MPC_T, 0]}}], set={"expert": lanes(2, SMALL), "labels": labels(1, SMALL)}),
           env=ENV, method="check_expert_state", **STEPPER)
)


def main():
    import ddpg_trucktrailer_amd          # (first: the replay code's conftest puts this tree's root in front of the path)
    from test_loop_refusals_cpu import TABLE, outcome
    commit = sys.argv[1] if len(sys.argv) > 1 else "the working tree"
    table = [dict(c, outcome=outcome(c)) for c in CASES]
    keys = [json.dumps({k: v for k, v in c.items() if k != "outcome"}, sort_keys=True) for c in table]
    assert len(set(keys)) == len(keys), [k for k in keys if keys.count(k) > 1]
    head = {"provenance": f"written by tests/golden/make_golden_loop_refusals.py from a git worktree of {commit}", "cases": None}
    with open(TABLE, "w") as f:
        f.write(json.dumps(head)[:-len("null}")] + "[\n" + ",\n".join(json.dumps(c) for c in table) + "\n]}\n")
    kinds = {}
    for c in table:
        kinds[c["outcome"][0]] = kinds.get(c["outcome"][0], 0) + 1
    print(f"{TABLE}: {len(table)} cases {kinds} from {os.path.dirname(ddpg_trucktrailer_amd.__file__)}")


if __name__ == "__main__":
    main()
