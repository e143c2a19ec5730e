"""What the GPU tests share and torch is needed for: the device fixture, output arrays with guard rows, arrays at the header's minimum alignment between
guard bytes (Fenced) and the comparison of bit patterns (bits, same) of the learner tests, the packed event counters,
the env and oracle constructors of the parity tests, the sentinel-filled, guarded output arrays of a rollout launch, and the runner of
one oc_rollout_random launch beside the oracle.  Imported like helpers.py; tests/case_support.py holds what needs no torch."""
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


GUARD_BYTES, GUARD_BYTE = 64, 0xEE  # the guard bytes on either side of a Fenced array, and what they hold
_TORCH = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.int32): torch.int32, np.dtype(np.uint8): torch.uint8}


class Fenced:
    """A device copy of numpy array `a` between GUARD_BYTES guard bytes on either side, its first byte `align` bytes behind a multiple
    of 2 * align: the minimum alignment include/oc_amd.h allows, which a fresh allocation never has."""

    def __init__(self, a, align, dev):
        a = np.ascontiguousarray(a)
        self.raw = torch.full((a.nbytes + 2 * GUARD_BYTES + 4 * align,), GUARD_BYTE, dtype=torch.uint8, device=dev)
        self.off = GUARD_BYTES + (align - (self.raw.data_ptr() + GUARD_BYTES)) % (2 * align)
        self.nbytes = a.nbytes
        part = self.raw[self.off:self.off + a.nbytes]
        part.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()))  # (a byte copy: NaN payloads arrive as they are)
        self.t = part.view(_TORCH[a.dtype]).view(a.shape)
        assert self.t.data_ptr() % (2 * align) == align % (2 * align)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def host(self):
        return self.t.cpu().numpy()

    def intact(self):
        return bool((self.raw[:self.off] == GUARD_BYTE).all()) and bool((self.raw[self.off + self.nbytes:] == GUARD_BYTE).all())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def same(x, y):
    return np.array_equal(bits(x), bits(y))


def guards_untouched(case, what, guards, fill):
    """Every guard row of the array `what` still holds `fill`."""
    if not all(bool((g == fill).all()) for g in guards):
        pytest.fail("%s: guard rows of the %s written" % (getattr(case, "id", case), what))


# The fills of a rollout's output arrays: values no result holds.  Rewards are sums of non-negative shaping and delivery rewards, a flag
# byte holds the OC_F_* bits (<= 7), an event mask has a bit per event kind and player (50 of 64).
REW_FILL, FLAG_FILL, MASK_FILL = -7.0, 0xEE, -1


class RolloutOutputs:
    """The rewards, flags and (masks=True) per-step event masks of one launch of `steps` steps of `n` envs, every element a sentinel
    and with guard rows on both sides.  The first output byte sits where include/oc_amd.h still allows it and a fresh allocation
    never does: the rewards 48 bytes behind the allocation's base (16-byte aligned, not 64), tiled flags 24 bytes behind it (8-byte
    aligned, not 16), [step][env] flags — written a byte at a time by every kernel — 3 bytes behind it (an odd address)."""

    def __init__(self, steps, n, device, tiled=False, masks=False, outputs=True):
        self.tiled, self.rew, self.fl, self.ev, self.guards = tiled, None, None, None, []
        if outputs:
            self._rewards_and_flags(steps, n, device, tiled)
        if masks:
            ev, g_ev = guarded(steps * n, (), torch.int64, MASK_FILL, device, before=GUARD)
            self.ev = ev.view(steps, n)
            self.guards.append(("event masks", g_ev, MASK_FILL))

    def _rewards_and_flags(self, steps, n, device, tiled):
        rew, g_rew = guarded(steps * n, (4,), torch.float32, REW_FILL, device, before=3)
        if tiled:
            fl, g_fl = guarded(steps // 8 * n, (8,), torch.uint8, FLAG_FILL, device, before=3)
            assert steps % 8 == 0 and fl.data_ptr() % 16 == 8
        else:
            fl, g_fl = guarded(steps * n, (), torch.uint8, FLAG_FILL, device, before=3)
            assert fl.data_ptr() % 2 == 1
        assert rew.data_ptr() % 64 == 48
        self.rew, self.fl = rew.view(steps, n, 4), fl.view(steps // 8, n, 8) if tiled else fl.view(steps, n)
        self.guards += [("rewards", g_rew, REW_FILL), ("flags", g_fl, FLAG_FILL)]

    def flags(self):
        """[steps, n], untiled where the launch wrote tiles"""
        from overcooked_ai_amd.vec_env import VecOvercookedEnv

        return VecOvercookedEnv.untile_flags(self.fl) if self.tiled else self.fl

    def guards_untouched(self, case):
        for what, g, fill in self.guards:
            guards_untouched(case, what, g, fill)

    def all_written(self, case):
        """No element still holds its sentinel: for launches that are compared with another launch, not with the oracle."""
        for what, t, fill in (("rewards", self.rew, REW_FILL), ("flags", self.fl, FLAG_FILL), ("event masks", self.ev, MASK_FILL)):
            if t is not None and bool((t == fill).any()):
                pytest.fail("%s: %d elements of the %s were not written" % (getattr(case, "id", case), int((t == fill).sum()), what))
        self.guards_untouched(case)


def record_buffers(K, n, n_planes, device, layouts=False, masks=False):
    """The arrays of a recorded launch of K steps (rollout_random's keywords -> tensor), every element a sentinel, and a function
    that fails where a guard row was written.  Guard rows behind every array; before it as far as its documented alignment allows:
    48 bytes before the recorded states and the rewards (16-byte aligned), 6 before the actions and the layout ids (2-byte aligned),
    3 before the flags."""
    out = RolloutOutputs(K, n, device, masks=masks)
    acts, g_acts = guarded(K * n, (2,), torch.uint8, 0xEE, device, before=3)
    states, g_states = guarded(K * n_planes * n, (16,), torch.uint8, 0xEE, device, before=3)
    assert states.data_ptr() % 64 == 48 and acts.data_ptr() % 4 == 2
    bufs = dict(actions_out=acts.view(K, n, 2), states_out=states.view(K, n_planes, n, 16), rewards_out=out.rew, flags_out=out.fl)
    guards = out.guards + [("recorded actions", g_acts, 0xEE), ("recorded states", g_states, 0xEE)]
    if masks:
        bufs["events_out"] = out.ev
    if layouts:
        lay, g_lay = guarded(K * n, (), torch.int16, -1, device, before=3)
        assert lay.data_ptr() % 4 == 2
        bufs["layouts_out"] = lay.view(K, n)
        guards.append(("recorded layout ids", g_lay, -1))

    def check(case):
        for what, g, fill in guards:
            guards_untouched(case, what, g, fill)
    return bufs, check


def _holds(values, fill):
    """`fill` is among the values (two cheap reductions settle it for every array of the oracle's: the fills lie outside their range)"""
    values = np.asarray(values)
    return values.size > 0 and values.min() <= fill <= values.max() and bool((values == fill).any())


def no_sentinel(case, rew_o=None, fl_o=None, masks_o=None):
    """The oracle's own results hold none of the fills: an element that still holds one was not written."""
    name = getattr(case, "id", case)
    assert rew_o is None or not _holds(rew_o, REW_FILL), "%s: an oracle reward equals the fill" % name
    assert fl_o is None or not _holds(fl_o, FLAG_FILL), "%s: an oracle flag byte equals the fill" % name
    assert masks_o is None or not _holds(np.asarray(masks_o).view(np.uint64), np.uint64(0xFFFFFFFFFFFFFFFF)), \
        "%s: an oracle event mask equals the fill" % name


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
    "lane_pair" / "predicate_interact", the env's switch to one of the opt-in rollout kernels.
    The output arrays are RolloutOutputs: sentinels between guard rows, off the base of their allocation; the guards must come back
    untouched, and no value of the oracle's equals a sentinel, so an element the launch did not write differs from the oracle's."""
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
    out = RolloutOutputs(steps, n, gpu, tiled=flags_tiled8, masks=events == 2, outputs=outputs)
    rew, fl, ev = out.rew, out.fl, out.ev
    what = "launch of %d envs x %d steps" % (n, steps)
    compare(what, t0, "first states", env.get_packed_state(), run.state, lid, env_axis=1)
    epoch = env.reset_epoch
    env.rollout_random(steps, rew, fl, events_out=ev, flags_tiled8=flags_tiled8)  # ONE call
    out.guards_untouched(what)
    if outputs:
        fl = out.flags()
    restarts = shaped = sparse = 0
    for c0, rew_o, fl_o, masks_o in run.chunks(steps, t0=t0, epoch=epoch):
        k = len(fl_o)
        no_sentinel(what, rew_o, fl_o, masks_o if ev is not None else None)
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
