"""oc_gae on the device: every case of tests/gae_cases.py against the numpy restatement of the header's arithmetic bit for bit, the
isolation a done step gives, the moments, and the collection loop — step_sampled(into=...) writing a TrajectoryBuffer's rows — against
an env stepped with plain calls whose outputs are copied."""
import ctypes

import numpy as np
import pytest
import torch

import gae_cases as GC
import partner_cases as PC
from gpu_support import GUARD, gpu, guarded, guards_untouched  # noqa: F401

pytestmark = pytest.mark.gpu

FILL = GC.FILL  # no advantage, target or sum of a case equals it (checked where it is used, and for every case without a GPU)
_TORCH = {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8}


def placed(a, align, dev):
    """A device copy of numpy array `a` (None stays None) whose first byte lies `align` bytes behind a multiple of 2 * align: the
    minimum alignment include/oc_amd.h allows, which a fresh allocation never has (align 1: an odd address)."""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    raw = torch.zeros((a.nbytes + 2 * align + 64,), dtype=torch.uint8, device=dev)
    off = align + (-raw.data_ptr()) % (2 * align)
    part = raw[off:off + a.nbytes]
    part.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8).copy()))  # (a byte copy: NaN payloads arrive as they are)
    t = part.view(_TORCH[a.dtype]).view(a.shape)
    assert t.data_ptr() % (2 * align) == align
    return t


def bits(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else t
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def run(what, dev, arrays, gamma, lam, moments=True, zero_last=False):
    """One oc_gae call through the C-ABI on placed inputs and sentinel-filled outputs between guard rows:
    (advantages, targets, partials, moments) as numpy arrays (the last two None without moments)."""
    from overcooked_ai_amd import _lib

    rewards, values, done, last, seat = arrays
    T, n = done.shape
    if zero_last:
        last = np.zeros((n, 2), np.float32)
    d_in = [placed(rewards, 16, dev), placed(values, 8, dev), placed(last, 8, dev), placed(done, 1, dev), placed(seat, 1, dev)]
    adv, g_adv = guarded(T * n, (2,), torch.float32, FILL, dev, before=GUARD)
    tgt, g_tgt = guarded(T * n, (2,), torch.float32, FILL, dev, before=GUARD)
    assert adv.data_ptr() % 16 == 8 and tgt.data_ptr() % 16 == 8
    blocks = (n + 255) // 256
    part = g_part = mom = g_mom = None
    if moments:
        part, g_part = guarded(blocks, (3,), torch.float64, FILL, dev, before=1)
        mom, g_mom = guarded(1, (3,), torch.float64, FILL, dev, before=1)
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    g = _lib.OcGaeBatch(*[ptr(t) for t in d_in], ptr(adv), ptr(tgt), ptr(part), ptr(mom), T, gamma, lam)
    b = _lib.OcBatch(n_envs=n)
    L = _lib.load()
    rc = L.oc_gae(ctypes.byref(b), ctypes.byref(g), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, L.oc_last_error().decode()
    torch.cuda.synchronize(dev)
    guards_untouched(what, "advantages", g_adv, FILL)
    guards_untouched(what, "targets", g_tgt, FILL)
    if moments:
        guards_untouched(what, "partials", g_part, FILL)
        guards_untouched(what, "moments", g_mom, FILL)
    return (adv.view(T, n, 2).cpu().numpy(), tgt.view(T, n, 2).cpu().numpy(), part.cpu().numpy() if moments else None,
            mom.view(3).cpu().numpy() if moments else None)


def check_moments(c, adv_ref, done, seat, part, mom):
    """The count exact, both sums within n * 2^-53 * sum |x| of numpy's float64 sums over the same entries, per 256-env block and
    for the whole; the whole is the sum of the partials in ascending order, bit for bit."""
    n = done.shape[1]
    assert part.shape == ((n + 255) // 256, 3)
    total = np.zeros(3)
    for k in range(len(part)):
        cnt, s1, s2, s_abs = GC.moments_f64(adv_ref, done, seat, 256 * k, 256 * k + 256)
        assert part[k, 0] == cnt, (c.id, k)
        assert abs(part[k, 1] - s1) <= cnt * 2.0 ** -53 * s_abs, (c.id, k, part[k, 1], s1)
        assert abs(part[k, 2] - s2) <= cnt * 2.0 ** -53 * s2, (c.id, k, part[k, 2], s2)  # (sum |A^2| is sum A^2)
        total = total + part[k]
    assert np.array_equal(bits(mom), bits(total)), (c.id, mom, total)
    cnt, s1, s2, s_abs = GC.moments_f64(adv_ref, done, seat)
    assert mom[0] == cnt and abs(mom[1] - s1) <= cnt * 2.0 ** -53 * s_abs and abs(mom[2] - s2) <= cnt * 2.0 ** -53 * s2, (c.id, mom)


@pytest.mark.parametrize("c", GC.CASES, ids=lambda c: c.id)
def test_every_case_equals_the_f32_restatement_bit_for_bit(c, gpu):
    arrays = GC.arrays_of(c)
    ref_adv, ref_tgt = GC.reference_of(c)
    assert not (ref_adv == FILL).any() and not (ref_tgt == FILL).any() and not np.isnan(ref_adv).any() and not np.isnan(ref_tgt).any()
    adv, tgt, part, mom = run(c.id, gpu, arrays, c.gamma, c.lam)
    for what, got, want in (("advantages", adv, ref_adv), ("targets", tgt, ref_tgt)):
        diff = bits(got) != bits(want)  # (zero tolerance; the sign of a zero included)
        if diff.any():
            t, e, p = (int(x[0]) for x in np.nonzero(diff))
            pytest.fail("%s: %d %s differ, first at step %d env %d player %d: %r, expected %r"
                        % (c.id, int(diff.sum()), what, t, e, p, float(got[t, e, p]), float(want[t, e, p])))
    check_moments(c, ref_adv, arrays[2], arrays[4], part, mom)
    # the same call without moments writes the same outputs
    adv2, tgt2, _, _ = run(c.id, gpu, arrays, c.gamma, c.lam, moments=False)
    assert np.array_equal(bits(adv2), bits(adv)) and np.array_equal(bits(tgt2), bits(tgt))


ISOLATION = [c for c in GC.CASES if c.done in ("horizon5", "random7", "first") and c.n_steps > GC.prefetch_block()][:6]


@pytest.mark.parametrize("c", ISOLATION, ids=lambda c: c.id)
def test_nan_behind_a_done_step_does_not_reach_it(c, gpu):
    """values[t + 1], and every reward and value behind it, of an env that is done at step t are NaN (the next episode, which is
    not compared): the outputs at and before step t are those of the clean run, bit for bit.  A kernel that multiplies by
    (1 - done) where the header selects gives NaN there."""
    clean_adv, clean_tgt = GC.reference_of(c)
    arrays, keep = GC.poisoned(c)
    assert (~keep).any() and keep.any()
    adv, tgt, _, _ = run(c.id, gpu, arrays, c.gamma, c.lam, moments=False)
    assert np.array_equal(bits(adv)[keep], bits(clean_adv)[keep]) and np.array_equal(bits(tgt)[keep], bits(clean_tgt)[keep])
    assert np.isnan(adv[~keep]).any()  # (the poison was where the kernel reads)


def test_moments_repeat_bit_for_bit_and_leave_out_every_partner_sample(gpu):
    c = next(c for c in GC.CASES if c.n_envs == 488 and c.n_steps == 2 * GC.prefetch_block() + 1)
    arrays = GC.arrays_of(c)
    first, second = run(c.id, gpu, arrays, c.gamma, c.lam), run(c.id, gpu, arrays, c.gamma, c.lam)
    for a, b in zip(first, second):
        assert np.array_equal(bits(a), bits(b))
    assert len(first[2]) == 2 and first[3][0] > 0
    # all-partner seats: every sample of player p is the partner's (a seat byte names one player of an env, so the other player's
    # samples are what is left): +0.0f outputs for p, and count and sums over the other player alone
    rewards, values, done, last, _ = arrays
    T, n = done.shape
    for p in (0, 1):
        seat = np.full((T, n), p, np.uint8)
        adv, tgt, part, mom = run(c.id, gpu, (rewards, values, done, last, seat), c.gamma, c.lam)
        assert not bits(adv[:, :, p]).any() and not bits(tgt[:, :, p]).any()
        assert mom[0] == T * n
        check_moments(c, adv, done, seat, part, mom)


def test_no_steps_or_no_envs_launch_nothing_and_zero_the_moments(gpu):
    """The one way to a count of 0: a batch without a sample.  The moments asked for are zeros, the partials of the envs there are
    too, and nothing else is written."""
    from overcooked_ai_amd import _lib

    L = _lib.load()
    n = 65
    for T, envs in ((0, n), (3, 0)):
        part, g_part = guarded(max((envs + 255) // 256, 1), (3,), torch.float64, FILL, gpu, before=1)
        mom, g_mom = guarded(1, (3,), torch.float64, FILL, gpu, before=1)
        buf = torch.full((64,), FILL, dtype=torch.float64, device=gpu)
        g = _lib.OcGaeBatch(buf.data_ptr(), buf.data_ptr(), None, buf.data_ptr(), None, buf.data_ptr(), buf.data_ptr(), part.data_ptr(),
                            mom.data_ptr(), T, 0.99, 0.98)
        b = _lib.OcBatch(n_envs=envs)
        assert L.oc_gae(ctypes.byref(b), ctypes.byref(g), torch.cuda.current_stream(gpu).cuda_stream) == 0, L.oc_last_error().decode()
        torch.cuda.synchronize(gpu)
        assert not bits(mom).any() and bool((buf == FILL).all())
        assert (not bits(part).any()) if envs else bool((part == FILL).all())
        guards_untouched("T=%d n=%d" % (T, envs), "partials", g_part, FILL)
        guards_untouched("T=%d n=%d" % (T, envs), "moments", g_mom, FILL)


def test_no_last_values_is_a_zero_array(gpu):
    c = next(c for c in GC.CASES if not c.last)
    arrays = GC.arrays_of(c)
    assert arrays[3] is None
    a, b = run(c.id, gpu, arrays, c.gamma, c.lam), run(c.id, gpu, arrays, c.gamma, c.lam, zero_last=True)
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))


def test_the_python_entry_point(gpu):
    from overcooked_ai_amd.gae import gae

    c = next(c for c in GC.CASES if c.n_envs == 257 and c.seat != "none")
    rewards, values, done, last, seat = GC.arrays_of(c)
    ref_adv, ref_tgt = GC.reference_of(c)
    dev = lambda a: torch.from_numpy(a.copy()).to(gpu) if a is not None else None  # noqa: E731
    adv, tgt, mom = gae(dev(rewards), dev(values), dev(done), c.gamma, c.lam, last_values=dev(last), seat=dev(seat), moments=True)
    assert np.array_equal(bits(adv), bits(ref_adv)) and np.array_equal(bits(tgt), bits(ref_tgt))
    cnt = GC.moments_f64(ref_adv, done, seat)[0]
    assert mom.shape == (3,) and mom.dtype == torch.float64 and float(mom[0]) == cnt
    T, n = done.shape
    out_a, g_a = guarded(T * n, (2,), torch.float32, FILL, gpu, before=GUARD)
    out_t, g_t = guarded(T * n, (2,), torch.float32, FILL, gpu, before=GUARD)
    got = gae(dev(rewards), dev(values), dev(done), c.gamma, c.lam, last_values=dev(last), seat=dev(seat),
              out=(out_a.view(T, n, 2), out_t.view(T, n, 2)))
    assert len(got) == 2 and got[0].data_ptr() == out_a.data_ptr() and np.array_equal(bits(got[0]), bits(ref_adv))
    assert np.array_equal(bits(got[1]), bits(ref_tgt))
    guards_untouched(c.id, "advantages", g_a, FILL)
    guards_untouched(c.id, "targets", g_t, FILL)
    with pytest.raises(ValueError):
        gae(dev(rewards), dev(values).cpu(), dev(done), c.gamma, c.lam)


# ------------------------------------------------------------------------------------------ the collection loop
STEPS, HORIZON = 12, 5


def _env(n, dev, policy):
    from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent

    env = VecOvercookedMultiAgent("cramped_room", n, horizon=HORIZON, obs="features", device=dev, seed=31, reward_shaping_factor=1.0,
                                  use_phi=True, bc_policy=policy)
    if policy is not None:
        env.set_bc_factor(0.5)
    return env


def _logits(n, t):
    return (np.random.default_rng(1000 + t).standard_normal((n, 2, 6)) * 2).astype(np.float32)


def _values(n, t):
    return (np.random.default_rng(2000 + t).uniform(-5, 5, (n, 2))).astype(np.float32)


@pytest.mark.parametrize("partner", (False, True), ids=("self_play", "bc_partner"))
@pytest.mark.parametrize("n", (65, 488))
def test_the_step_writes_the_buffer_rows_it_is_given(n, partner, gpu):
    from overcooked_ai_amd.partner import DensePolicy
    from overcooked_ai_amd.trajectory_buffer import TrajectoryBuffer

    policy = DensePolicy(*PC.glorot(5, PC.total_of(2), 64, 64), device=gpu) if partner else None
    plain, direct, mixed = _env(n, gpu, policy), _env(n, gpu, policy), _env(n, gpu, policy)
    buf, buf_mixed = TrajectoryBuffer(direct, STEPS), TrajectoryBuffer(mixed, STEPS)
    assert (buf.seat is not None) == partner
    for env in (plain, direct, mixed):
        env.reset()
    direct.shaped.fill_(FILL)  # the persistent buffers of the env that only ever steps into rows: never written
    direct.done.fill_(0xEE)
    copies = []
    for t in range(STEPS):
        lg = [torch.from_numpy(_logits(n, t)).to(gpu) for _ in range(3)]
        values = torch.from_numpy(_values(n, t)).to(gpu)
        obs_p, shaped_p, done_p, infos_p = plain.step_sampled(lg[0])
        copy = dict(rewards=shaped_p.clone(), done=done_p.clone(), actions=infos_p["actions"].clone(), logp=infos_p["logp"].clone(),
                    seat=infos_p["seat"].clone() if partner else None, obs=obs_p.clone())
        copies.append(copy)
        assert shaped_p.data_ptr() == plain.shaped.data_ptr() and done_p.data_ptr() == plain.done.data_ptr()
        # ---- every step into its row
        row = buf.row(t, values)
        obs_d, shaped_d, done_d, infos_d = direct.step_sampled(lg[1], into=row)
        assert shaped_d.data_ptr() == buf.rewards[t].data_ptr() and done_d.data_ptr() == buf.done[t].data_ptr()
        assert infos_d["actions"].data_ptr() == buf.actions[t].data_ptr() and infos_d["logp"].data_ptr() == buf.logp[t].data_ptr()
        assert np.array_equal(bits(obs_d), bits(copy["obs"])), t
        assert np.array_equal(bits(lg[1]), bits(lg[0])), t  # (the partner wrote the same logits)
        # ---- plain and into calls taking turns (plain, into, into, plain, ...): every call seats and steps as the all-plain env does
        if t % 3 == 0:
            obs_m, shaped_m, done_m, infos_m = mixed.step_sampled(lg[2])
            assert shaped_m.data_ptr() == mixed.shaped.data_ptr() and mixed._last_done is mixed.done
        else:
            obs_m, shaped_m, done_m, infos_m = mixed.step_sampled(lg[2], into=buf_mixed.row(t, values))
            assert shaped_m.data_ptr() == buf_mixed.rewards[t].data_ptr() and mixed._last_done.data_ptr() == buf_mixed.done[t].data_ptr()
        got = dict(rewards=shaped_m, done=done_m, actions=infos_m["actions"], logp=infos_m["logp"],
                   seat=infos_m["seat"] if partner else None, obs=obs_m)
        for key, want in copy.items():
            if want is not None:
                assert np.array_equal(got[key].cpu().numpy().view(np.uint8), want.cpu().numpy().view(np.uint8)), (t, key)
        assert bool(done_p.all()) == (t % HORIZON == HORIZON - 1)
    assert bool((direct.shaped == FILL).all()) and bool((direct.done == 0xEE).all())
    assert direct.done.data_ptr() != direct._last_done.data_ptr() and direct.sample_step == plain.sample_step == STEPS
    for key in ("rewards", "done", "actions", "logp") + (("seat",) if partner else ()):
        want = torch.stack([c[key] for c in copies])
        assert np.array_equal(getattr(buf, key).cpu().numpy().view(np.uint8), want.cpu().numpy().view(np.uint8)), key
    assert np.array_equal(bits(buf.values), bits(np.stack([_values(n, t) for t in range(STEPS)])))
    if partner:
        seats = buf.seat.cpu().numpy()
        assert (seats != 255).any() and (seats == 255).any() and (seats[1:] != seats[:-1]).any()
    assert bool((buf.rewards != 0).any()) and bool((buf.done != 0).any())
    # ---- the advantages of the buffer
    buf.last_values.copy_(torch.from_numpy(_values(n, STEPS)).to(gpu))
    adv, tgt, mom = buf.advantages(0.99, 0.98)
    seat = buf.seat.cpu().numpy() if partner else None
    ref_adv, ref_tgt = GC.gae_f32(buf.rewards.cpu().numpy(), buf.values.cpu().numpy(), buf.done.cpu().numpy(), 0.99, 0.98,
                                  buf.last_values.cpu().numpy(), seat)
    assert np.array_equal(bits(adv), bits(ref_adv)) and np.array_equal(bits(tgt), bits(ref_tgt))
    count, s1, s2 = (float(x) for x in mom)
    assert count == GC.moments_f64(ref_adv, buf.done.cpu().numpy(), seat)[0] and s2 > 0
    with pytest.raises(ValueError):
        direct.step_sampled(lg[1], into=buf.row(0, values)._replace(done=buf.done[0][:-1]))
    with pytest.raises(ValueError):
        direct.step_sampled(lg[1], into=buf.row(0, values)._replace(logp=buf.logp[0].double()))
    assert direct.sample_step == STEPS  # (refused before anything was drawn)
