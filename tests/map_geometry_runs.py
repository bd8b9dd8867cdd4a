"""TEST INFRASTRUCTURE: the worlds of tests/map_geometry_scenes.py as oracle configurations and runs -- what
tests/test_map_geometry.py (the oracle) and the GPU tests off the square grid (the device against it) both start from."""
import numpy as np

import map_geometry_scenes as mg
import ref
from helpers import keti_thresholds
from nav_gym_amd import abi

STEPS = 12
SHAPES = [(85, 330), (330, 85), (96, 203), (203, 96)]
ORIGINS = [(-16.0, 32.0), (-7.3, 12.9)]

# Pedestrian state under translation is not bit-exact: the social force adds metres at another magnitude.  Worst deviation
# of the un-shifted state over the runs of test_translation_identity_with_pedestrians (both origins, 6 arenas x 3 pedestrians
# x 13 observations), measured on the oracle; bound = 4 x worst, one digit (DESIGN.md section 5 sets its bounds that way):
#   positions 1.51e-14 m, velocities 5.50e-15 m/s, yaw 1.72e-14 rad   (origin (-16, 32); at (-7.3, 12.9): 5.3e-15, 2.3e-15, 5.7e-15)
# (An ulp of a position near 34 m is 7.1e-15 m.  The oracle's sin / cos / atan2 / exp are its own, so the figures do not
# depend on the machine's libm.)
PED_SHIFT_BOUND = dict(ped_xy=6e-14, ped_vel=2e-14, ped_yaw=7e-14)


def config(H, W, E=6, n_beams=181, ped_model=abi.PED_NONE, N=3, **kw):
    kw = dict(dict(n_envs=E, n_beams=n_beams, map_h=H, map_w=W, max_peds=N, ped_model=ped_model, n_scan_stack=2,
                   auto_reset=1, n_spawn=4, max_waypoints=4, seed=11), **kw)
    cfg = ref.default_config(**kw)
    cfg.angle_min, cfg.angle_last = -0.75 * np.pi, 0.75 * np.pi
    return cfg


def run(cfg, world, steps=STEPS, seed=5, v_scale=1.0):
    r = ref.RefSim(cfg, world)
    cmd = None
    if cfg.ped_model == abi.PED_EXTERNAL:
        def cmd(t, rng):
            r.set_ped_cmd(np.stack([rng.uniform(0, 0.6, (cfg.n_envs, cfg.max_peds)),
                                    rng.uniform(-0.6, 0.6, (cfg.n_envs, cfg.max_peds))], axis=2))
    state = lambda: {k: r.a[k] for k in mg.STATE if k in r.a}
    return mg.rollout(r.reset_obs, r.step, state, cfg.n_envs, steps, seed, v_scale, cmd), r


def scene(H, W, ped_model=abi.PED_NONE, inside=True, kind="closed", seed=3, **kw):
    cfg = config(H, W, ped_model=ped_model, **kw)
    occ = mg.make_maps(cfg.n_envs, H, W, seed, kind)
    world = mg.make_world(cfg, occ, ref.build_dt(occ), keti_thresholds(cfg), seed, n_peds=0 if ped_model == abi.PED_NONE else cfg.max_peds,
                          inside=inside)
    return cfg, occ, world


def ped_shift_deviation(cfg, rec, cfg_t, rec_t, label="pedestrians"):
    covered, dev = mg.check_translation(cfg, rec, cfg_t, rec_t, label, scans=False)
    assert covered == cfg.n_envs * (STEPS + 1)
    return {k: dev[k] for k in PED_SHIFT_BOUND}


PED_TRANSLATION_SEED = 3
