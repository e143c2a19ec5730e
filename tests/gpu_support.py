"""What the GPU tests share and torch is needed for: the device fixture, output arrays with guard rows, the packed event counters,
the env and oracle constructors of the parity tests, and the runner of one oc_rollout_random launch beside the oracle.  Imported like helpers.py; tests/case_support.py holds what needs no torch."""
import numpy as np
import pytest
import torch

from case_support import compare, new_oracle

GUARD = 3  # guard rows behind (and, where asked, before) an output array


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from overcooked_ai_amd import _lib

    _lib.load()  # fail loudly if the HIP extension is missing
    return torch.device("cuda:0")


def guarded(rows, row_shape, dtype, fill, device, before=0):
    """(rows [before, before + rows) of a new array of before + rows + GUARD rows, all of it `fill`, a value no result holds; its
    guard slices: the rows behind the output and, with before > 0, those before it)."""
    whole = torch.full((before + rows + GUARD,) + tuple(row_shape), fill, dtype=dtype, device=device)
    return whole[before:before + rows], (whole[before + rows:],) + ((whole[:before],) if before else ())


def guards_untouched(case, what, guards, fill):
    """Every guard row of the array `what` still holds `fill`."""
    if not all(bool((g == fill).all()) for g in guards):
        pytest.fail("%s: guard rows of the %s written" % (getattr(case, "id", case), what))


def packed_counters(t):
    """[n_envs, 25] int32, player 0 in the low half-word -> [n_envs, 25, 2]"""
    c = t.cpu().numpy().astype(np.int64)
    return np.stack([c & 0xFFFF, (c >> 16) & 0xFFFF], -1)


def make_env(layouts, n, gpu, **kw):
    from overcooked_ai_amd.vec_env import VecOvercookedEnv

    return VecOvercookedEnv(layouts, n, device=gpu, **kw)


def oracle_for(specs):
    return new_oracle(specs if isinstance(specs, (list, tuple)) else [specs])


def long_launch_against_oracle(gpu, table, n, lid=None, env_offset=0, seed=0, steps=4000, horizon=400, start=None,
                                flags_tiled8=False, one_wavefront=False, expect_shaped=True, t0=0, outputs=True, events=0,
                                regen_layout=False, expect=None, epoch0=None, option=None, **env_kw):
    """flags_tiled8: the launch writes the OC_OPT_FLAGS_TILED8 layout (the instances bench.py times), untiled before the
    comparison; one_wavefront: OC_OPT_ONE_WAVEFRONT (no mover / interact split where the batch would get it); t0: the launch's
    first global step; outputs=False: no rewards / flags arrays — states, returns and counters are compared all the same;
    events: 1 per-episode counters (running and published), 2 also the per-step masks, against the popcounts of the oracle's
    event_infos; regen_layout: every restart re-draws the env's layout, the ids are compared; expect: the instance
    oc_rollout_plan must name for exactly this call, asked on this device before the launch; epoch0: the epoch the launch starts
    from (the env's own counter, set after its construction: the first states are drawn at epoch 0 all the same); option: None, or
    "lane_pair" / "predicate_interact", the env's switch to one of the opt-in rollout kernels."""
    import rollout_cases as RC
    from overcooked_ai_amd.vec_env import VecOvercookedEnv

    env = VecOvercookedEnv(table, n, horizon=horizon, device=gpu, auto_reset=True, seed=seed, env_offset=env_offset,
                           layout_id=lid, track_events=events > 0, regen_layout=regen_layout, **env_kw)
    env.one_wavefront = one_wavefront
    env.t_global = t0
    if epoch0 is not None:
        env._epoch = epoch0
    if option is not None:
        setattr(env, option, True)
    assert bool(start) == env.random_starts, "start must name the env's own start_state_fn keywords"
    if expect is not None:
        plan = RC.plan_of(env.table, n, steps, t0, horizon, tiled=flags_tiled8, one_wavefront=one_wavefront, outputs=outputs,
                       events=events, start=start, regen=env.regen, seed=seed, env_offset=env_offset, epoch=env.reset_epoch, option=option)
        assert plan.startswith(expect), "this launch is planned as\n  %s\nnot as\n  %s" % (plan, expect)
    run = RC.OracleLaunch(env.table.specs, n, layout_id=lid, seed=seed, env_offset=env_offset, horizon=horizon, start=start,
                       regen=env.regen, events=events > 0)
    rew = torch.zeros((steps, n, 4), dtype=torch.float32, device=gpu) if outputs else None
    fl = torch.zeros((steps // 8, n, 8) if flags_tiled8 else (steps, n), dtype=torch.uint8, device=gpu) if outputs else None
    ev = torch.zeros((steps, n), dtype=torch.int64, device=gpu) if events == 2 else None
    what = "launch of %d envs x %d steps" % (n, steps)
    compare(what, t0, "first states", env.get_packed_state(), run.state, lid, env_axis=1)
    epoch = env.reset_epoch
    env.rollout_random(steps, rew, fl, events_out=ev, flags_tiled8=flags_tiled8)  # ONE call
    if flags_tiled8:
        fl = VecOvercookedEnv.untile_flags(fl)
    restarts = shaped = sparse = 0
    for c0, rew_o, fl_o, masks_o in run.chunks(steps, t0=t0, epoch=epoch):
        k = len(fl_o)
        if outputs:
            # ([step][env]...: the step a message names is the chunk's first, the index it gives starts with the step inside the chunk)
            compare(what, c0, "flags of steps %d..%d" % (c0, c0 + k), fl[c0:c0 + k].cpu().numpy(), fl_o, lid, env_axis=1)
            compare(what, c0, "rewards of steps %d..%d" % (c0, c0 + k), rew[c0:c0 + k].cpu().numpy(), rew_o, lid, env_axis=1)
        if ev is not None:
            compare(what, c0, "event masks of steps %d..%d" % (c0, c0 + k), ev[c0:c0 + k].cpu().numpy().view(np.uint64), masks_o, lid, env_axis=1)
        restarts += int(((fl_o & 4) != 0).sum())
        sparse += float(rew_o[..., :2].sum())
        shaped += float(rew_o[..., 2:].sum())
    last = t0 + steps - 1
    if env.regen is not None:
        compare(what, last, "layout ids", env.layout_ids(), run.layout_id, None)
    compare(what, last, "final states", env.get_packed_state(), run.state, lid, env_axis=1)
    compare(what, last, "episode returns", env.ep_returns.cpu().numpy(), run.ep_returns, lid)
    if events:
        compare(what, last, "running event counters", packed_counters(env.event_counts), run.counts, lid)
        compare(what, last, "published event counters", packed_counters(env.event_counts_done), run.counts_done, lid)
        assert run.counts_done.sum() > 0
    assert restarts == n * (steps // horizon) and (shaped > 0 or not expect_shaped)
    return sparse, shaped
