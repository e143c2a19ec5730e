"""oc_outcome_table on the device: every case of tests/outcome_cases.py through the C-ABI — arrays at the header's minimum alignments
between guard bytes, sentinel-filled outputs, a scratch of the planned size — against the numpy restatement of the header's order bit
for bit and against the float64 reference that knows no order; then the collection loop (step_sampled(into=...) writing the episode
returns and the members into a TrajectoryBuffer's rows), evaluate() and PartnerPool.set_weights on a live env."""
import ctypes

import numpy as np
import pytest
import torch

import outcome_cases as OC
import partner_cases as PC
import pool_cases as PP
from gpu_support import Fenced, bits, gpu, same  # noqa: F401

pytestmark = pytest.mark.gpu

FILL = OC.FILL


def run(what, dev, arrays, junk, per_env=True):
    """One oc_outcome_table call through the C-ABI: done, seat and member at odd addresses, ep_returns 16-byte and not 32-byte
    aligned, the outputs and the scratch 8-byte and not 16-byte aligned, all between guard bytes; the outputs start as FILL, the
    scratch as `junk`.  (table, env_table or None, scratch as [blocks, G + 1, 8]) as numpy arrays."""
    from overcooked_ai_amd import _lib

    done, ep, seat, member, K = arrays
    T, n = done.shape
    G = OC.n_groups(seat, K)
    nbytes = OC.scratch_bytes(n, T, seat is not None, member is not None, K)
    assert nbytes % ((G + 1) * 64) == 0
    d_in = [Fenced(done, 1, dev), Fenced(ep, 16, dev), Fenced(seat, 1, dev) if seat is not None else None,
            Fenced(member, 1, dev) if member is not None else None]
    table = Fenced(np.full((G + 1, 8), FILL), 8, dev)
    env = Fenced(np.full((n, 4), FILL), 8, dev) if per_env else None
    scratch = Fenced(np.full((nbytes // 8,), junk), 8, dev)
    assert d_in[0].ptr % 2 == 1 and d_in[1].ptr % 32 == 16 and table.ptr % 16 == 8 and scratch.ptr % 16 == 8
    ptr = lambda f: f.ptr if f is not None else None  # noqa: E731
    q = _lib.OcOutcomeBatch(*[ptr(f) for f in d_in], table.ptr, ptr(env), scratch.ptr, n, T, K)
    L = _lib.load()
    rc = L.oc_outcome_table(ctypes.byref(q), torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0, L.oc_last_error().decode()
    torch.cuda.synchronize(dev)
    for name, f in (("done", d_in[0]), ("ep_returns", d_in[1]), ("seat", d_in[2]), ("member", d_in[3]), ("table", table), ("env table", env),
                    ("scratch", scratch)):
        assert f is None or f.intact(), "%s: guard bytes of the %s written" % (what, name)
    for f, a in zip(d_in, (done, ep, seat, member)):
        assert f is None or same(f.host(), a), "%s: an input was written" % what
    return table.host(), env.host() if per_env else None, scratch.host().reshape(-1, G + 1, 8)


def first_difference(what, name, got, want):
    diff = bits(got) != bits(want)
    if diff.any():
        at = tuple(int(x[0]) for x in np.nonzero(diff))
        pytest.fail("%s: %d entries of the %s differ, first at %r: %r, expected %r" % (what, int(diff.sum()), name, at, float(got[at]), float(want[at])))


@pytest.mark.parametrize("c", OC.CASES, ids=lambda c: c.id)
def test_every_case_equals_the_restatement_bit_for_bit_and_the_reference_within_its_bound(c, gpu):
    arrays = OC.arrays_of(c)
    want_table, want_env, want_partials = OC.restated_of(c)
    ref_table, ref_env, mags, env_mags = OC.reference_of(c)
    table, env, scratch = run(c.id, gpu, arrays, np.nan)
    assert not (table == FILL).any() and not (env == FILL).any()  # every entry was written
    # ---- the header's order, every float64 by its bit pattern: the table, the env table and the partials in the scratch
    first_difference(c.id, "table", table, want_table)
    first_difference(c.id, "env table", env, want_env)
    first_difference(c.id, "partials", scratch, want_partials)
    # ---- the reference that knows no order
    if c.kind == "integer":  # every sum is exact: zero tolerance whatever the order
        first_difference(c.id, "table (reference)", table, ref_table)
        first_difference(c.id, "env table (reference)", env, ref_env)
    else:
        assert OC.within_bound(table, ref_table, ref_table[:, :1], mags)[:, OC.SUM_COLS].all(), c.id
        assert OC.within_bound(env, ref_env, ref_env[:, :1], env_mags).all(), c.id
    for col in (0, OC.MIN_COL, OC.MAX_COL):  # counts, min and max are exact; the unattributed count is in column 0 of the last row
        first_difference(c.id, "column %d" % col, table[:, col], ref_table[:, col])
    first_difference(c.id, "env episodes", env[:, 0], ref_env[:, 0])
    empty = ref_table[:-1, 0] == 0
    assert same(table[:-1][empty], np.broadcast_to(OC.empty_table(1)[0], (int(empty.sum()), 8)))  # 0 / +inf / -inf
    assert same(table[-1, 1:], OC.empty_table(1)[0, 1:])
    assert table[:, 0].sum() == np.count_nonzero(arrays[0])
    # ---- a second call on a scratch of other contents, and one without the env table: the same bytes
    again, _, scratch2 = run(c.id, gpu, arrays, 1e300, per_env=False)
    assert same(again, table) and same(scratch2, scratch), c.id


def test_488_envs_are_200_and_288(gpu):
    """Counts, min and max do not depend on how a batch is cut: the table of 488 envs against those of its first 200 and its last
    288 envs."""
    c = next(c for c in OC.CASES if (c.n_envs, c.n_steps, c.kind, c.member, c.done, c.seat) == (488, 400, "real", "k3", "sparse", "mixed"))
    done, ep, seat, member, K = OC.arrays_of(c)
    whole, env, _ = run(c.id, gpu, (done, ep, seat, member, K), np.nan)
    parts = [run(c.id, gpu, tuple(np.ascontiguousarray(a[:, lo:hi]) for a in (done, ep, seat, member)) + (K,), np.nan)
             for lo, hi in ((0, 200), (200, 488))]
    (a, env_a, _), (b, env_b, _) = parts
    assert same(whole[:, 0], a[:, 0] + b[:, 0]) and whole[:, 0].min() > 0
    assert same(whole[:, OC.MIN_COL], np.fmin(a[:, OC.MIN_COL], b[:, OC.MIN_COL])) and same(whole[:, OC.MAX_COL], np.fmax(a[:, OC.MAX_COL], b[:, OC.MAX_COL]))
    assert same(env, np.concatenate([env_a, env_b]))  # (an env's own sums do not know its neighbours)


def test_no_envs_write_the_empty_table(gpu):
    from overcooked_ai_amd import _lib
    from overcooked_ai_amd.outcomes import outcome_table

    L = _lib.load()
    for seat, member, K in ((False, False, 1), (True, False, 1), (True, True, 2)):
        G = 1 + 2 * K if seat else 1
        table = Fenced(np.full((G + 1, 8), FILL), 8, gpu)
        hold = torch.zeros((64,), dtype=torch.uint8, device=gpu)
        q = _lib.OcOutcomeBatch(None, None, hold.data_ptr() if seat else None, hold.data_ptr() if member else None, table.ptr, None, None, 0, 3, K)
        assert L.oc_outcome_table(ctypes.byref(q), torch.cuda.current_stream(gpu).cuda_stream) == 0, L.oc_last_error().decode()
        torch.cuda.synchronize(gpu)
        assert table.intact() and same(table.host(), OC.empty_table(G + 1)) and not hold.any()
    done = torch.zeros((3, 0), dtype=torch.uint8, device=gpu)
    out = outcome_table(done, torch.zeros((3, 0, 4), device=gpu), seat=done, member=done, n_members=2, per_env=True)
    assert same(out.table.cpu().numpy(), OC.empty_table(6)) and out.env_table.shape == (0, 4) and out.episodes == 0


def test_the_python_entry_point(gpu):
    from overcooked_ai_amd.outcomes import outcome_table

    c = next(c for c in OC.CASES if c.n_envs == 257 and c.member == "k3" and c.seat == "mixed" and c.kind == "real")
    done, ep, seat, member, K = OC.arrays_of(c)
    want_table, want_env, _ = OC.restated_of(c)
    dev = lambda a: torch.from_numpy(a.copy()).to(gpu) if a is not None else None  # noqa: E731
    out = outcome_table(dev(done), dev(ep), seat=dev(seat), member=dev(member), n_members=K, per_env=True)
    assert out.table.dtype == torch.float64 and tuple(out.table.shape) == (2 * K + 2, 8) and out._host is None  # (nobody has waited)
    assert same(out.table.cpu().numpy(), want_table) and same(out.env_table.cpu().numpy(), want_env)
    ref = OC.reference_of(c)[0]
    assert out.episodes == int(ref[:-1, 0].sum()) and out.unattributed == int(ref[-1, 0]) > 0
    assert out.min == ref[:-1, OC.MIN_COL].min() and out.max == ref[:-1, OC.MAX_COL].max()
    assert abs(out.mean - ref[:-1, 1].sum() / ref[:-1, 0].sum()) <= 1e-9 and out.std > 0
    by = out.by_member()
    assert same(by["episodes"], ref[1:-1, 0].reshape(K, 2)) and by["mean"].shape == (K, 2)
    plain = outcome_table(dev(done), dev(ep))
    assert tuple(plain.table.shape) == (2, 8) and plain.env_table is None and plain.episodes == np.count_nonzero(done) and plain.unattributed == 0
    one = outcome_table(dev(done), dev(ep), seat=dev(seat))  # one partner policy: every valid seat is member 0's
    assert tuple(one.table.shape) == (4, 8) and one.by_member()["episodes"].shape == (1, 2)
    with pytest.raises(ValueError):
        outcome_table(dev(done), dev(ep).cpu())


# ------------------------------------------------------------------------------------------ the collection loop
N_ENVS, HORIZON, STEPS = 130, 7, 25
SENTINEL = -3.0


def _pool(dev):
    from overcooked_ai_amd.partner import DensePolicy, PartnerPool

    return PartnerPool([DensePolicy(*PC.glorot(40 + m, PC.total_of(2), *PP.SHAPES[m]), device=dev) for m in range(3)])


def _env(dev, pool, bc_factor, n=N_ENVS):
    from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent

    env = VecOvercookedMultiAgent("cramped_room", n, horizon=HORIZON, obs="features", device=dev, seed=77, reward_shaping_factor=1.0, use_phi=True,
                                  bc_policy=pool, random_start_pos=True, rnd_obj_prob_thresh=0.9)  # (drawn starts: objects in hand, pots in use)
    env.set_bc_factor(bc_factor)
    return env


def _logits(n, t):
    return (np.random.default_rng(3000 + t).standard_normal((n, 2, 6)) * 2).astype(np.float32)


def _bytes(t):
    return t.cpu().numpy().view(np.uint8)


@pytest.mark.parametrize("bc_factor", (0.5, 1.0))
def test_the_step_writes_the_returns_and_members_of_the_rows_it_is_given(bc_factor, gpu):
    from overcooked_ai_amd.trajectory_buffer import TrajectoryBuffer

    pool = _pool(gpu)
    plain, direct, mixed = (_env(gpu, pool, bc_factor) for _ in range(3))
    buf, buf_mixed = TrajectoryBuffer(direct, STEPS, keep_returns=True), TrajectoryBuffer(mixed, STEPS, keep_returns=True)
    assert tuple(buf.ep_returns.shape) == (STEPS, N_ENVS, 4) and buf.ep_returns.dtype == torch.float32 and buf.member.dtype == torch.uint8
    assert TrajectoryBuffer(direct, 2).ep_returns is None and TrajectoryBuffer(direct, 2).row(0, buf.values[0]).ep_returns is None
    for env in (plain, direct, mixed):
        env.reset()
    direct.ep_returns.fill_(SENTINEL)  # the persistent buffer of the env that only ever steps into rows: never written
    values = torch.zeros((N_ENVS, 2), device=gpu)
    clones = []
    for t in range(STEPS):
        lg = [torch.from_numpy(_logits(N_ENVS, t)).to(gpu) for _ in range(3)]
        _, _, done_p, infos_p = plain.step_sampled(lg[0])
        assert infos_p["ep_returns"].data_ptr() == plain.ep_returns.data_ptr()
        clone = dict(ep_returns=infos_p["ep_returns"].clone(), done=done_p.clone(), seat=infos_p["seat"].clone(), member=infos_p["member"].clone())
        clones.append(clone)
        row = buf.row(t, values)
        assert row.ep_returns.data_ptr() == buf.ep_returns[t].data_ptr() and row.ep_returns.data_ptr() % 16 == 0
        _, _, done_d, infos_d = direct.step_sampled(lg[1], into=row)
        assert infos_d["ep_returns"].data_ptr() == buf.ep_returns[t].data_ptr() and done_d.data_ptr() == buf.done[t].data_ptr()
        # ---- plain and into calls taking turns
        if t % 3 == 0:
            _, _, done_m, infos_m = mixed.step_sampled(lg[2])
            got = dict(ep_returns=infos_m["ep_returns"], done=done_m, seat=infos_m["seat"], member=infos_m["member"])
            assert infos_m["ep_returns"].data_ptr() == mixed.ep_returns.data_ptr()
        else:
            mixed.step_sampled(lg[2], into=buf_mixed.row(t, values))
            got = dict(ep_returns=buf_mixed.ep_returns[t], done=buf_mixed.done[t], seat=buf_mixed.seat[t], member=buf_mixed.member[t])
        for key, want in clone.items():
            assert np.array_equal(_bytes(got[key]), _bytes(want)), (t, key)
        assert bool(done_p.all()) == (t % HORIZON == HORIZON - 1)
    assert bool((direct.ep_returns == SENTINEL).all())
    stacked = {key: torch.stack([c[key] for c in clones]) for key in clones[0]}
    for key, want in stacked.items():  # the rows are the clones, byte for byte
        assert np.array_equal(_bytes(getattr(buf, key)), _bytes(want)), key
    host = {key: t.cpu().numpy() for key, t in stacked.items()}
    assert (host["member"] == 255).any() == (bc_factor < 1) and set(np.unique(host["member"])) - {255} == {0, 1, 2}
    assert ((host["member"] == 255) == (host["seat"] == 255)).all()
    # ---- the table of the buffer: the numpy table of the clones, exactly (the env's returns are integers)
    out = buf.outcomes(per_env=True)
    ref_table, ref_env, _, _ = OC.reference(host["done"], host["ep_returns"], host["seat"], host["member"], 3)
    rows = host["ep_returns"][host["done"] != 0]
    assert (rows == np.round(rows)).all()  # (integers: every sum is exact)
    print("bc_factor %r: %d episodes, returns summed over them %r" % (bc_factor, len(rows), rows.sum(axis=0).tolist()))
    first_difference("bc_factor %r" % bc_factor, "table", out.table.cpu().numpy(), ref_table)
    first_difference("bc_factor %r" % bc_factor, "env table", out.env_table.cpu().numpy(), ref_env)
    assert out.episodes == N_ENVS * (STEPS // HORIZON) and out.unattributed == 0
    by = out.by_member()
    assert by["episodes"].sum() + ref_table[0, 0] == out.episodes and (by["episodes"] > 0).all()
    assert (ref_table[0, 0] == 0) == (bc_factor == 1.0)
    assert same(out.env_table[:, 0].cpu().numpy(), np.full(N_ENVS, float(STEPS // HORIZON)))
    with pytest.raises(ValueError):
        TrajectoryBuffer(direct, 2).outcomes()
    with pytest.raises(ValueError):
        direct.step_sampled(lg[1], into=buf.row(0, values)._replace(ep_returns=buf.ep_returns[0][:, :3]))
    with pytest.raises(ValueError):
        direct.step_sampled(lg[1], into=buf.row(0, values)._replace(member=buf.member[0][:-1]))
    assert direct.sample_step == STEPS  # (refused before anything was drawn)


def _act(dev, width):
    w = torch.from_numpy(np.random.default_rng(5).standard_normal((width, 6)).astype(np.float32) * 0.3).to(dev)
    return lambda obs: (obs.float() @ w).contiguous()


def test_evaluate_is_the_table_of_the_same_steps_collected_by_hand(gpu):
    from overcooked_ai_amd.outcomes import evaluate

    pool = _pool(gpu)
    env, by_hand = _env(gpu, pool, 1.0), _env(gpu, pool, 1.0)
    act = _act(gpu, PC.total_of(2))
    out = evaluate(env, act, episodes=2)
    obs = by_hand.reset()
    cols = dict(done=[], ep_returns=[], seat=[], member=[])
    for t in range(2 * HORIZON):
        obs, _, done, infos = by_hand.step_sampled(act(obs))
        for key, t_ in (("done", done), ("ep_returns", infos["ep_returns"]), ("seat", infos["seat"]), ("member", infos["member"])):
            cols[key].append(t_.clone())
    host = {key: torch.stack(v).cpu().numpy() for key, v in cols.items()}
    ref_table = OC.reference(host["done"], host["ep_returns"], host["seat"], host["member"], 3)[0]
    first_difference("evaluate", "table", out.table.cpu().numpy(), ref_table)
    assert out.episodes == N_ENVS * 2 and out.unattributed == 0 and ref_table[0, 0] == 0  # bc_factor 1: a row of a cross-play table
    assert out.by_member()["episodes"].sum() == N_ENVS * 2 and env.sample_step == 2 * HORIZON
    greedy = evaluate(env, act, episodes=1, greedy=True)
    assert greedy.episodes == N_ENVS
    with pytest.raises(ValueError):
        evaluate(env, act, episodes=0)


def test_set_weights_moves_the_draw_from_the_next_call_on(gpu):
    pool = _pool(gpu)
    env = _env(gpu, pool, 1.0)
    env.reset()
    thr = PP.uniform_thresholds(3)
    v = env.venv
    seat = member = done = None
    pool.set_weights([0, 0, 1])
    for t in range(3 * HORIZON + 1):
        if t == 3:
            pool.set_weights([1, 0, 0])  # mid-episode: nobody is reseated until the episode ends
        if t == 2 * HORIZON - 2:
            pool.set_weights(None)
        step = env.sample_step
        _, _, d, infos = env.step_sampled(torch.from_numpy(_logits(N_ENVS, t)).to(gpu))
        got_seat, got_member = infos["seat"].cpu().numpy(), infos["member"].cpu().numpy()
        episode = t // HORIZON
        if episode == 0:
            assert (got_member == 2).all(), t  # all weight on member 2
        elif episode == 1:
            assert (got_member == 0).all(), t  # every newly seated partner is member 0
        else:  # uniform again: the draws of a pool built uniform
            if t % HORIZON == 0:
                want_seat, want_member = PP.redraw(seat, member, done, v.seed, v.env_offset, step, 1.0, thr)
                assert np.array_equal(got_seat, want_seat) and np.array_equal(got_member, want_member)
                assert set(np.unique(got_member)) == {0, 1, 2}
            else:
                assert np.array_equal(got_member, member)
        seat, member, done = got_seat, got_member, d.cpu().numpy().copy()
