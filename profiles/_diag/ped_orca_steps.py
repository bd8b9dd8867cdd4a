"""c3-shaped world (4096 arenas, 20 pedestrians, 1081 beams, 500 x 500 maps) through NavGymEnv.step() with three pedestrian
models: 'sfm', 'orca' (navsim_ped_orca: one kernel on the simulator's state) and 'compose' -- what a user had before that
entry existed: torch gathers of the [E N, N + 1, 6] agent lists, navsim_crowd_orca, step(human_actions=...).  Prints
env-steps/s per variant (NAVSIM_VARIANTS=sfm,orca,compose picks some).  Under rocprofv3 --kernel-trace --stats with
NAVSIM_VARIANTS=orca it gives ped_orca_kernel's own time (profiles/r08_orca/)."""
import os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "nav-gym_amd"))
import torch, nav_gym_env
from nav_gym_amd import sim as simmod

E = int(os.environ.get("NAVSIM_ENVS", "4096"))
N = int(os.environ.get("NAVSIM_PEDS", "20"))
K, Wm = int(os.environ.get("NAVSIM_STEPS", "200")), 30
DEV = "cuda:0"


def compose(env, p, order):
    """ped_cmd of the ORCA model out of the state tensors, on the host's side of the C ABI (two waypoint pops at most)."""
    t, cfg = env.sim.t, env.sim.cfg
    pose, vel, n = t["ped_pose"], t["ped_vel"], t["n_peds"].long()
    head, nwp, wps = t["ped_wp_head"].long(), t["ped_n_waypoints"].long(), t["ped_waypoints"]
    for _ in range(2):
        w = torch.gather(wps, 2, head[..., None, None].expand(E, N, 1, 2))[:, :, 0]
        d = pose[..., :2] - w
        head = head + ((torch.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) < 1.0) & (head + 1 < nwp)).long()
    g = torch.gather(wps, 2, head[..., None, None].expand(E, N, 1, 2))[:, :, 0] - pose[..., :2]
    s = torch.sqrt(g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1])
    pref = torch.where((s > 1.0)[..., None], g / s[..., None], g)
    vp = t["ped_v_pref"]
    row = torch.cat([pose[..., :2], vel, torch.full((E, N, 1), (p["ped_radius"] + 0.01) + p["safety_space"], dtype=torch.float64,
                                                    device=DEV)], dim=2)                      # [E,N,5]
    ag = row[:, order]                                                                         # [E,N,N,5]: self, the others ascending
    rp, pv = t["robot_pose"], t["prev_action"][:, 0]
    rob = torch.stack([rp[:, 0], rp[:, 1], pv * torch.cos(rp[:, 2]), pv * torch.sin(rp[:, 2]),
                       torch.full((E,), (p["robot_radius"] + 0.01) + p["safety_space"], dtype=torch.float64, device=DEV)], dim=1)
    ag = torch.cat([ag, rob[:, None, None, :].expand(E, N, 1, 5)], dim=2)                      # [E,N,N+1,5]
    # ragged arenas: the robot follows the live pedestrians directly
    ag = ag.scatter(2, n[:, None, None, None].expand(E, N, 1, 5), rob[:, None, None, :].expand(E, N, 1, 5))
    ag = torch.cat([ag, vp[..., None, None].expand(E, N, N + 1, 1)], dim=3).reshape(E * N, N + 1, 6)
    _, act = simmod.crowd_orca({k: p[k] for k in simmod.ORCA_KEYS}, ag, pref.reshape(-1, 2),
                               n_agents=(n + 1)[:, None].expand(E, N).reshape(-1), theta=pose[..., 2].reshape(-1))
    return torch.stack([act[:, 0], act[:, 1] / cfg.time_step], dim=1).reshape(E, N, 2)


def run(variant):
    env = nav_gym_env.make("NavGym-v0", num_envs=E, n_beams=1081, map_size=500, indoor_ratio=0.0, device=DEV, seed=1234,
                           pedestrian_model="external" if variant == "compose" else variant, num_humans=N, plan_paths=False)
    env.reset()
    g = torch.Generator(device=DEV); g.manual_seed(78)
    acts = torch.rand((K + Wm, E, 2), generator=g, device=DEV, dtype=torch.float64)
    acts[..., 0] *= 0.5; acts[..., 1] = acts[..., 1] * 1.28 - 0.64
    p = simmod.ped_orca_defaults(env.sim.cfg, env.robot_type)
    idx = torch.arange(N, device=DEV)
    order = torch.stack([torch.cat([idx[i:i + 1], idx[:i], idx[i + 1:]]) for i in range(N)])   # [N,N]

    def step(a):
        if variant == "compose":
            env.step(a, human_actions=compose(env, p, order))
        else:
            env.step(a)
    for t in range(Wm):
        step(acts[t])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(K):
        step(acts[Wm + t])
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    print("%-8s %.3f M env-steps/s, %.4f ms per step" % (variant, E * K / el / 1e6, el / K * 1e3), flush=True)
    env.close()
    return E * K / el


rates = {v: run(v) for v in os.environ.get("NAVSIM_VARIANTS", "sfm,orca,compose").split(",")}
if "orca" in rates and "compose" in rates:
    print("orca / compose: %.2f x" % (rates["orca"] / rates["compose"]))
