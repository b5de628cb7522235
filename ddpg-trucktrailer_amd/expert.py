"""Expert-transition ingestion: trainv2.py:457-466 re-inserts stored transitions
`(obs, action, reward, obs_next, done)` one `agent.remember` call at a time; exp_gen.py:77-110 produces them with
the action already divided by radians(45).  Here they are loaded in bulk into the device replay memory:

  * `load_into_replay(buffer, ...)`  -- the per-transition `ReplayBuffer` the reference-style `Agent.learn()` samples;
  * `load_into_ring(ring, ...)`      -- the side buffer of the `TrajectoryRing` the N-env loop samples: expert tuples are
    not steps of any env's trajectory, so they sit next to the time-major ring and `tt_ring_sample` draws uniformly over
    ring transitions and side transitions together (the reference draws uniformly over one buffer that holds both);
  * `save_transitions_npz` / `load_transitions_npz` -- the five arrays as one .npz file (tools/train_vector.py --demos)."""
import numpy as np


def transitions_to_arrays(stored_transitions):
    """list of episodes, each a list of (obs, action, reward, obs_next, done) -> five arrays."""
    rows = [t for episode in stored_transitions for t in episode]
    obs = np.stack([np.asarray(t[0], np.float32) for t in rows])
    act = np.stack([np.asarray(t[1], np.float32).reshape(-1) for t in rows])
    rew = np.array([float(t[2]) for t in rows], np.float32)
    obs2 = np.stack([np.asarray(t[3], np.float32) for t in rows])
    done = np.array([bool(t[4]) for t in rows], np.bool_)
    return obs, act, rew, obs2, done


def load_into_replay(buffer, stored_transitions):
    """Bulk version of the `agent.remember` loop of trainv2.py:462-465; returns the number loaded."""
    obs, act, rew, obs2, done = transitions_to_arrays(stored_transitions)
    buffer.store_batch(obs, act, rew, obs2, done)
    return len(rew)


def load_into_ring(ring, stored_transitions, capacity=None):
    """The same transitions into the N-env loop's replay (TrajectoryRing.load_side); returns the number loaded.
    Loops holding captured hipGraphs of the sampling launch re-capture afterwards (ring.side_epoch moves)."""
    obs, act, rew, obs2, done = transitions_to_arrays(stored_transitions)
    return ring.load_side(obs, act[:, 0], rew, obs2, done, capacity=capacity)


_NPZ_KEYS = ("obs", "act", "rew", "obs2", "done")


def save_transitions_npz(path, obs, act, rew, obs2, done):
    """The five arrays of transitions_to_arrays (obs [k,23] f32, act [k,1] f32, rew [k] f32, obs2 [k,23] f32, done [k] bool) as one
    .npz file: what tools/train_vector.py --demos reads."""
    obs, obs2 = np.asarray(obs, np.float32), np.asarray(obs2, np.float32)
    k = obs.shape[0]
    act, rew, done = np.asarray(act, np.float32).reshape(k, -1), np.asarray(rew, np.float32).reshape(k), np.asarray(done).astype(np.bool_).reshape(k)
    if obs.ndim != 2 or obs2.shape != obs.shape or act.shape != (k, 1):
        raise ValueError(f"transitions of shapes obs {obs.shape}, act {act.shape}, obs2 {obs2.shape} are not [k, d], [k, 1], [k, d]")
    with open(path, "wb") as f:
        np.savez(f, obs=obs, act=act, rew=rew, obs2=obs2, done=done)
    return k


def load_transitions_npz(path):
    """(obs, act, rew, obs2, done) of a file save_transitions_npz wrote, with the dtypes and shapes of transitions_to_arrays."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in _NPZ_KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{path}: no array named {', '.join(missing)} (a demonstration file holds obs, act, rew, obs2, done)")
        obs, act, rew, obs2, done = (z[k] for k in _NPZ_KEYS)
    k = obs.shape[0]
    if obs.ndim != 2 or obs2.shape != obs.shape or act.reshape(k, -1).shape != (k, 1) or rew.shape != (k,) or done.shape != (k,):
        raise ValueError(f"{path}: shapes obs {obs.shape}, act {act.shape}, rew {rew.shape}, obs2 {obs2.shape}, done {done.shape} do not "
                         "belong to one set of transitions")
    return (obs.astype(np.float32), act.astype(np.float32).reshape(k, 1), rew.astype(np.float32), obs2.astype(np.float32),
            done.astype(np.bool_))
