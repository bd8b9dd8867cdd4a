"""TEST INFRASTRUCTURE (GPU): navsim_rollout_obs through the C ABI into sentinel-filled outputs, and the step itself as its
reference: the saved state and observation put back, H navsim_step calls with sequence k -- each call's observation the next
call's obs_prev, as NavSim.step chains them -- and everything they wrote stacked, for tests/test_gpu_rollout_obs.py.  The state's
save and restore are tests/lookahead_call.py's."""
import ctypes as C

import numpy as np

import lookahead_call as lc
from gpu_support import same_bits, to_device
from nav_gym_amd import abi

KEYS = tuple(abi.ROLLOUT_OBS_OUT)
SHARED = tuple(abi.ROLLOUT_OUT)                                             # what navsim_rollout returns too
ALL = ("obs_all", "goals_all")


def call(gpu, cfg, st, actions, obs_prev, noise=abi.LOOKOBS_NOISE_STEP, gamma=1.0, ped_cmd=None, skip=None, rows="all"):
    """navsim_rollout_obs into sentinel-filled outputs -> NumPy arrays.  actions: [E,K,H,2] float64; obs_prev: the device tensor
    [E,D] the next step would read; rows 'last': out.obs_all / goals_all are NULL and the dict has neither."""
    torch, E = gpu.torch, cfg.n_envs
    actions = np.ascontiguousarray(actions, np.float64)
    K, H = actions.shape[1:3]
    sym = {"K": K, "H": H, "D": cfg.n_scan_stack * cfg.n_beams + abi.OBS_TAIL}
    out = {}
    for k, (dtype, tail) in abi.ROLLOUT_OBS_OUT.items():
        if k in ALL and rows != "all":
            continue
        shape = (E,) + tuple(sym.get(s, s) for s in tail)
        out[k] = torch.full(shape, 77, dtype=getattr(torch, dtype), device=gpu.dev)
    o = abi.NavsimRolloutObsOut(**{k: v.data_ptr() for k, v in out.items()})
    p = abi.NavsimRolloutObsParams(n_seq=K, horizon=H, noise=int(noise), gamma=float(gamma))
    t_act = to_device(gpu, actions)
    t_cmd = None if ped_cmd is None else to_device(gpu, np.ascontiguousarray(ped_cmd, np.float64))
    t_skip = None if skip is None else to_device(gpu, np.asarray(skip, np.uint8))
    rc = gpu.lib.load().navsim_rollout_obs(C.byref(cfg), C.byref(st), C.byref(p), t_act.data_ptr(),
                                           None if t_cmd is None else t_cmd.data_ptr(),
                                           None if obs_prev is None else obs_prev.data_ptr(),
                                           None if t_skip is None else t_skip.data_ptr(), C.byref(o), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def steps_of(gpu, g, saved, obs0, actions, ped_cmd=None):
    """For every sequence k: the saved state and the observation obs0 put back, then H navsim_step calls with actions[:, k, h] ->
    what they wrote, stacked [E,K,H,...]: reward, done, is_success, is_crash, distance, limit (io.truncated, or done without
    success and crash), pose (the state's robot_pose behind the step: the scan pose unless the step crashed or restarted), obs,
    goals (achieved | desired) and, with NavSim(final_obs=True), final_obs / final_goals.  State and observation are put back."""
    E, K, H = actions.shape[:3]
    out = {}
    for k in range(K):
        lc.load_state(g, saved)
        g.obs.copy_(obs0)
        if ped_cmd is not None:
            g.set_ped_cmd(ped_cmd)
        seq = {}
        for h in range(H):
            row, o = g.step(to_device(gpu, actions[:, k, h]))
            got = {name: o[name] for name in lc.STEP_KEYS}
            got["limit"] = o["truncated"] if "truncated" in o else o["done"] & (o["is_success"] == 0) & (o["is_crash"] == 0)
            got["pose"] = g.t["robot_pose"]
            got["obs"] = row
            got["goals"] = gpu.torch.cat([o["achieved_goal"], o["desired_goal"]], dim=1)
            if g.final is not None:
                got.update(g.final)
            for name, v in got.items():
                seq.setdefault(name, []).append(v.cpu().numpy().copy())
        for name, v in seq.items():
            out.setdefault(name, []).append(np.stack(v, axis=1))
    lc.load_state(g, saved)
    g.obs.copy_(obs0)
    return {name: np.stack(v, axis=1) for name, v in out.items()}


def expected_length(step):
    """[E,K]: index of the first done step + 1, else H."""
    done = step["done"] != 0
    H = done.shape[2]
    return np.where(done.any(axis=2), done.argmax(axis=2) + 1, H).astype(np.int32)


def same_as_steps(roll, step, what, gamma=1.0, final=False):
    """Rule 5 against the step's own results: for every row h < min(length, exact_steps) reward, pose (where the step did not
    crash or restart), the observation row and the goals; behind `length` zeros; the last evaluated step's outcome, distance,
    obs_last and goals_last when it is an exact one.  final (same-step auto-reset): a done row is io.final_obs / final_goals.
    Returns the number of rows compared."""
    E, K, H = step["reward"].shape
    want_len = expected_length(step)
    exact = roll["exact_steps"]
    assert (roll["status"] == 1).all() and ((exact >= 1) & (exact <= H)).all()
    rows = 0
    for e in range(E):
        for k in range(K):
            L, X = int(roll["length"][e, k]), int(exact[e, k])
            n = min(L, X)
            tag = "%s: [%d,%d]" % (what, e, k)
            if X >= want_len[e, k]:
                assert L == want_len[e, k], "%s length %d, the step's %d" % (tag, L, want_len[e, k])
            same_bits(roll["reward"][e, k, :n], step["reward"][e, k, :n], tag + " reward")
            moved = (step["is_crash"][e, k, :n] != 0) | ((step["done"][e, k, :n] != 0) if final else False)
            same_bits(roll["pose"][e, k, :n][~moved], step["pose"][e, k, :n][~moved], tag + " pose")
            want_obs, want_goals = step["obs"][e, k], step["goals"][e, k]
            if final:
                done = step["done"][e, k] != 0
                want_obs = np.where(done[:, None], step["final_obs"][e, k], want_obs)
                want_goals = np.where(done[:, None], step["final_goals"][e, k], want_goals)
            if "obs_all" in roll:
                same_bits(roll["obs_all"][e, k, :n], want_obs[:n], tag + " rows")
                same_bits(roll["goals_all"][e, k, :n], want_goals[:n], tag + " goals")
                assert not roll["obs_all"][e, k, L:].any() and not roll["goals_all"][e, k, L:].any(), tag + " rows behind length"
            assert not roll["reward"][e, k, L:].any() and not roll["pose"][e, k, L:].any(), tag + " scalars behind length"
            rows += n
            if L - 1 < X:                                          # the last evaluated step is an exact one
                h = L - 1
                want = int(step["is_success"][e, k, h] != 0) | int(step["is_crash"][e, k, h] != 0) << 1 | int(step["limit"][e, k, h] != 0) << 2
                assert int(roll["outcome"][e, k]) == want, "%s outcome %d, the step's %d" % (tag, roll["outcome"][e, k], want)
                same_bits(roll["distance"][e, k], step["distance"][e, k, h], tag + " distance")
                same_bits(roll["obs_last"][e, k], want_obs[h], tag + " obs_last")
                same_bits(roll["goals_last"][e, k], want_goals[h], tag + " goals_last")
                ret, g_ = 0.0, 1.0                                 # float64, in the stated order
                for r in roll["reward"][e, k, :L]:
                    ret = ret + g_ * float(r)
                    g_ = g_ * float(gamma)
                same_bits(roll["ret"][e, k], np.float64(ret), tag + " ret")
                assert (roll["min_margin"][e, k] < 0) == bool((step["is_crash"][e, k, :L] != 0).any()), tag + " margin's sign"
            if "obs_all" in roll:
                same_bits(roll["obs_last"][e, k], roll["obs_all"][e, k, L - 1], tag + " obs_last against row length - 1")
                same_bits(roll["goals_last"][e, k], roll["goals_all"][e, k, L - 1], tag + " goals_last against row length - 1")
    return rows


def zero_rows(out, arenas, what):
    """Every array of the arenas' rows is 0 (status included)."""
    for name in out:
        assert not out[name][arenas].any(), "%s: %s" % (what, name)
