"""oc_outcome_table without a GPU: the exports and the struct against the header, the plan's words, every refusal (made before any
device call: this host has no device), the numpy restatement of the header's order against a scalar loop in rational arithmetic and
against the float64 reference that knows no order, the mutants of the header's sentences, the case list's own claims, and the Python
surface that needs no device: rank_weights, PartnerPool.set_weights, the TrajectoryRow defaults."""
import ctypes
import os
import re

import numpy as np
import pytest

import outcome_cases as OC
from case_support import P, ROOT

EINVAL = -1
WHO = "oc_outcome_table: "


def _header():
    with open(os.path.join(ROOT, "include", "oc_amd.h")) as f:
        return f.read()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------ the ABI
def test_exports_and_the_struct_match_the_header():
    from overcooked_ai_amd import _lib

    L = _lib.load()
    hdr = _header()
    for name in ("oc_outcome_table", "oc_outcome_plan"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    body = re.search(r"typedef struct OcOutcomeBatch \{(.*?)\} OcOutcomeBatch;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    Q = _lib.OcOutcomeBatch
    assert re.findall(r"\b(d_\w+|n_envs|n_steps|n_members)\b", body) == [f[0] for f in Q._fields_]
    assert [getattr(Q, f).offset for f, _ in Q._fields_] == list(range(0, 80, 8)) and ctypes.sizeof(Q) == 80
    assert "int oc_outcome_table(const OcOutcomeBatch* q, void* stream);" in hdr
    assert ("int oc_outcome_plan(int64_t n_envs, int64_t n_steps, int with_seat, int with_member, int n_members, int with_env_table, char* out,\n"
            "                    size_t out_size);") in hdr
    assert len(L.oc_outcome_table.argtypes) == 2 and len(L.oc_outcome_plan.argtypes) == 8
    assert L.oc_abi_version() == 6 and "#define OC_ABI_VERSION 6" in hdr


def test_the_header_states_what_the_restatement_restates():
    hdr = _header()
    for words in ("READ ONLY WHERE d_done IS SET", "group 1 + 2 m + s", "in ascending t and, within a step, in ascending e",
                  "the tables of its wavefronts q = 0, 1, 2, 3, in that order", "the partials b = 0, 1, ..., ceil(n_envs / B) - 1, in that order",
                  "No atomics on floating-point data", "Every sum\n * starts at +0.0", "slow, and correct", "what it held does not matter"):
        assert words in hdr, words


def _plan(n, T, seat=0, member=0, k=1, env=0, size=512):
    from overcooked_ai_amd import _lib

    L = _lib.load()
    out = ctypes.create_string_buffer(size)
    rc = L.oc_outcome_plan(n, T, seat, member, k, env, out, len(out))
    return rc, (out.value.decode() if rc == 0 else L.oc_last_error().decode())


def test_the_plan_in_words():
    hdr = _header()
    rc, text = _plan(65536, 400, 1, 1, 3)
    assert rc == 0 and text == ("k_outcomes<SEAT=true, MEMBER=true, ENV=false> grid=256, 256 lanes (one per env; one partial per block of 256 envs), "
                                "16 steps per prefetch block, 25 block(s) + k_outcome_sum grid=1, 64 lanes; G = 7 group(s), table 512 B, "
                                "scratch 131072 B"), text
    assert text in hdr
    rc, text = _plan(0, 5)
    assert rc == 0 and text == "k_outcome_sum grid=1, 64 lanes (no envs: the empty table); G = 1 group(s), table 128 B, scratch 0 B" and text in hdr
    B, D = OC.env_block(), OC.prefetch_block()
    assert B % 64 == 0 and D >= 2
    for n, T, seat, member, k, env in ((1, 1, 0, 0, 1, 0), (63, D - 1, 1, 0, 1, 1), (257, D, 1, 1, 1, 0), (488, D + 1, 1, 1, 16, 1), (2100, 400, 1, 1, 2, 0)):
        rc, text = _plan(n, T, seat, member, k, env)
        G = 1 + 2 * k if seat else 1
        blocks = (n + B - 1) // B
        m = re.fullmatch(r"k_outcomes<SEAT=(true|false), MEMBER=(true|false), ENV=(true|false)> grid=(\d+), (\d+) lanes \(one per env; one partial "
                         r"per block of (\d+) envs\), (\d+) steps per prefetch block, (\d+) block\(s\) \+ k_outcome_sum grid=1, 64 lanes; "
                         r"G = (\d+) group\(s\), table (\d+) B, scratch (\d+) B", text)
        assert rc == 0 and m, text
        assert m.groups() == tuple(str(x) for x in (("false", "true")[seat], ("false", "true")[member], ("false", "true")[env], blocks, B, B, D,
                                                    (T + D - 1) // D, G, (G + 1) * 64, blocks * (G + 1) * 64)), text
        assert OC.scratch_bytes(n, T, seat, member, k) == blocks * (G + 1) * 64
    rc, msg = _plan(5, 5, size=0)
    assert rc == EINVAL and msg.startswith("oc_outcome_plan: no output buffer")
    from overcooked_ai_amd import outcomes

    assert outcomes.plan(65536, 400, True, True, 3) == _plan(65536, 400, 1, 1, 3)[1]
    assert outcomes.scratch_bytes(2100, 7, True, True, 16) == 9 * 34 * 64 and outcomes.n_groups(True, 16) == 33 and outcomes.n_groups(False) == 1


SHAPE_REFUSALS = (
    (dict(T=0), "n_steps < 1"), (dict(T=-3), "n_steps < 1"), (dict(n=-1), "n_envs < 0"),
    (dict(n=2**16, T=2**15), "n_steps * n_envs must be below 2^31"), (dict(n=2**31, T=1), "n_steps * n_envs must be below 2^31"),
    (dict(n=3, T=2**62), "n_steps * n_envs must be below 2^31"), (dict(seat=0, member=1), "d_member needs d_seat"),
    (dict(k=0), "n_members must be in 1..16"), (dict(k=17), "n_members must be in 1..16"), (dict(k=-1), "n_members must be in 1..16"),
    (dict(member=0, k=2), "n_members must be 1 without d_member"), (dict(seat=0, member=0, k=2), "n_members must be 1 without d_member"),
)


@pytest.mark.parametrize("change,why", SHAPE_REFUSALS, ids=[w[1].replace(" ", "_") + str(i) for i, w in enumerate(SHAPE_REFUSALS)])
def test_every_refusal_of_a_shape_by_the_plan_and_by_the_call(change, why):
    """OC_EINVAL with the entry point's name in front, from oc_outcome_plan and from oc_outcome_table alike, before any device call
    (there is no device here: a call that got as far as a launch would not return OC_EINVAL)."""
    from overcooked_ai_amd import _lib

    L = _lib.load()
    a = dict(n=65, T=9, seat=1, member=1, k=3)
    a.update(change)
    rc, msg = _plan(a["n"], a["T"], a["seat"], a["member"], a["k"])
    assert rc == EINVAL and msg.startswith(WHO + why), msg
    q = _lib.OcOutcomeBatch(P, P, P if a["seat"] else None, P if a["member"] else None, P, None, P, a["n"], a["T"], a["k"])
    assert L.oc_outcome_table(ctypes.byref(q), None) == EINVAL and L.oc_last_error().decode().startswith(WHO + why)
    assert _plan(2**15, 2**16 - 1, 1, 1, 3)[0] == 0  # (one env row below 2^31)


ARRAY_REFUSALS = (
    (dict(d_done=None), "NULL d_done, d_ep_returns or d_scratch"), (dict(d_ep_returns=None), "NULL d_done, d_ep_returns or d_scratch"),
    (dict(d_scratch=None), "NULL d_done, d_ep_returns or d_scratch"), (dict(d_table=None), "NULL d_table"),
    (dict(d_table=None, n_envs=0), "NULL d_table"),
    (dict(d_ep_returns=P + 8), "d_ep_returns must be 16-byte aligned"), (dict(d_ep_returns=P + 4), "d_ep_returns must be 16-byte aligned"),
    (dict(d_table=P + 4), "d_table, d_env_table and d_scratch must be 8-byte aligned"),
    (dict(d_env_table=P + 12), "d_table, d_env_table and d_scratch must be 8-byte aligned"),
    (dict(d_scratch=P + 1), "d_table, d_env_table and d_scratch must be 8-byte aligned"),
    (dict(d_seat=None), "d_member needs d_seat"),
)


@pytest.mark.parametrize("change,why", ARRAY_REFUSALS, ids=[w[1].split(" must")[0].replace(" ", "_").replace(",", "") + str(i) for i, w in enumerate(ARRAY_REFUSALS)])
def test_every_refusal_of_an_array(change, why):
    from overcooked_ai_amd import _lib

    L = _lib.load()
    q = _lib.OcOutcomeBatch(P + 1, P + 16, P + 3, P + 5, P + 8, P + 8, P + 8, 65, 9, 3)  # (the minimum alignments: accepted as far as the checks go)
    for name, value in change.items():
        setattr(q, name, value)
    assert L.oc_outcome_table(ctypes.byref(q), None) == EINVAL
    assert L.oc_last_error().decode().startswith(WHO + why), L.oc_last_error().decode()
    assert L.oc_outcome_table(None, None) == EINVAL and L.oc_last_error().decode().startswith(WHO + "batch is NULL")


# ------------------------------------------------------------------------------------------ the case list's own claims
def test_the_case_list_covers_what_it_says():
    cs = OC.CASES
    D = OC.prefetch_block()
    assert len({c.id for c in cs}) == len(cs) and len(cs) <= 90
    assert {c.n_envs for c in cs} == {1, 63, 64, 65, 255, 256, 257, 488, 2100}
    for n in OC.SIZES:
        assert {c.n_steps for c in cs if c.n_envs == n} >= {1, D - 1, D, D + 1, 400}, n
    for kind in OC.KINDS:
        assert {c.done for c in cs if c.kind == kind} == set(OC.DONE_PATTERNS), kind
        assert {(c.seat, c.member) for c in cs if c.kind == "real"} >= {(s, m) for s in OC.SEAT_PATTERNS[1:] for m in OC.MEMBER_PATTERNS}
    assert any(c.seat == "none" for c in cs) and any(c.invalid for c in cs) and any(not c.invalid and c.seat == "mixed" for c in cs)
    assert any(c.n_envs == 2100 and c.kind == "real" and c.n_steps == 400 for c in cs)
    for c in cs:
        done, ep, seat, member, K = OC.arrays_of(c)
        T, n = c.n_steps, c.n_envs
        assert done.shape == (T, n) and ep.shape == (T, n, 4) and done.dtype == np.uint8 and ep.dtype == np.float32
        assert np.isnan(ep[done == 0]).all() and not np.isnan(ep[done != 0]).any(), c.id  # the poison, and none of it where a row is read
        assert (seat is None) == (c.seat == "none") and (member is None) == (c.member == "none") and K == OC.MEMBERS_OF[c.member]
        if c.kind == "integer" and (done != 0).any():
            rows = ep[done != 0].astype(np.float64)
            assert (rows[:, :2] % 20 == 0).all() and (rows == np.round(rows)).all() and rows.max() < 2**10, c.id
        if c.invalid and (done != 0).sum() > 200:
            assert OC.reference_of(c)[0][-1, 0] > 0, c.id  # (invalid bytes on done steps: an unattributed count)
        if c.done == "never":
            assert not done.any()
        if c.done == "every":
            assert done.all() and (done.size < 8 or (done != 1).any())  # (any non-zero byte)
    k16 = [c for c in cs if c.member == "k16" and c.done in ("sparse", "every", "equal") and c.n_envs >= 63]
    assert k16
    for c in k16:
        done, ep, seat, member, K = OC.arrays_of(c)
        t = OC.reference_of(c)[0]
        per_member = t[1:-1, 0].reshape(16, 2).sum(axis=1)
        assert (per_member[[m for m in range(16) if m not in OC.K16_DRAWN + (OC.K16_LONER,)]] == 0).all(), c.id  # empty members
        lone = (member == OC.K16_LONER) & (seat <= 1) & (done != 0)
        assert len(set(np.nonzero(lone)[1])) <= 1  # a member that appears in one env only
    assert any(((OC.arrays_of(c)[3] == OC.K16_LONER) & (OC.arrays_of(c)[2] <= 1) & (OC.arrays_of(c)[0] != 0)).any() for c in k16)


# ------------------------------------------------------------------------------------------ the restatement
INTEGER = [c for c in OC.CASES if c.kind == "integer"]
REAL = [c for c in OC.CASES if c.kind == "real"]


@pytest.mark.parametrize("c", INTEGER, ids=lambda c: c.id)
def test_the_restatement_is_a_rational_scalar_loop_on_the_integer_kind(c):
    """Every sum of the integer kind is exact in float64 (checked: the rational entries convert without rounding), so the
    restatement, the reference and the rational loop are ONE table, whatever the order."""
    arrays = OC.arrays_of(c)
    table, env, partials = OC.restated_of(c)
    want_table, want_env = OC.rational_table(*arrays)
    for row in want_table:
        assert all(x is None or (x.denominator == 1 and abs(x) < 2**53) for x in row)
    assert np.array_equal(bits(table), bits(OC.as_floats(want_table))), c.id
    assert np.array_equal(bits(env), bits(OC.as_floats(want_env))), c.id
    ref_table, ref_env, _, _ = OC.reference_of(c)
    assert np.array_equal(bits(table), bits(ref_table)) and np.array_equal(bits(env), bits(ref_env)), c.id
    assert partials.shape == ((c.n_envs + OC.env_block() - 1) // OC.env_block(),) + table.shape
    assert table[:, 0].sum() == np.count_nonzero(arrays[0])


@pytest.mark.parametrize("c", REAL, ids=lambda c: c.id)
def test_the_restatement_is_within_the_bound_of_the_reference_on_the_real_kind(c):
    """|restated - fsum| <= n * 2^-53 * sum |x| for every sum (n the group's or the env's episodes); counts, min and max equal."""
    table, env, _ = OC.restated_of(c)
    ref_table, ref_env, mags, env_mags = OC.reference_of(c)
    assert OC.within_bound(table, ref_table, ref_table[:, :1], mags)[:, OC.SUM_COLS].all(), c.id
    for col in (0, OC.MIN_COL, OC.MAX_COL):
        assert np.array_equal(bits(table[:, col]), bits(ref_table[:, col])), (c.id, col)
    assert OC.within_bound(env, ref_env, ref_env[:, :1], env_mags).all() and np.array_equal(env[:, 0], ref_env[:, 0]), c.id
    assert table[:, 0].sum() == np.count_nonzero(OC.arrays_of(c)[0])
    empty = ref_table[:-1, 0] == 0
    assert (table[:-1][empty] == OC.empty_table(1)[0]).all()  # 0 / +inf / -inf
    assert np.array_equal(bits(table[-1, 1:]), bits(OC.empty_table(1)[0, 1:]))  # the unattributed row: its count alone


MUTANTS = ("descending_partials", "lanes_before_steps", "drop_seat_bit", "read_a_step_early")


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_of_the_sentences_is_seen_by_a_case(mutant):
    """A kernel that adds its partials in descending order, takes a wavefront's episodes env by env, drops the seat bit of the group
    index or reads a row of a step that is not done differs from the statement in the bits of at least one case's table — so the GPU
    test, which compares bits, would see it."""
    pool = REAL if mutant in MUTANTS[:2] else OC.CASES
    if mutant == "read_a_step_early":  # (where every step is done, the step before holds a row too, not the poison)
        pool = [c for c in OC.CASES if c.done != "every"]
    seen = None
    for c in pool:
        if mutant == "descending_partials" and c.n_envs <= 2 * OC.env_block():  # (two partials add to the same bits either way)
            continue
        table, env, _ = OC.restated_of(c)
        m_table, m_env, _ = OC.restated(*OC.arrays_of(c), **{mutant: True})
        if not np.array_equal(bits(table), bits(m_table)):
            seen = c.id
            if mutant == "read_a_step_early":
                assert np.isnan(m_table).any() and np.isnan(m_env).any()  # (the poison is what it read)
            break
    assert seen, mutant


# ------------------------------------------------------------------------------------------ the Python surface without a device
def test_rank_weights_and_set_weights_are_held_to_thresholds_of():
    import partner_cases as PC
    import pool_cases as PP
    from overcooked_ai_amd.partner import DensePolicy, PartnerPool, rank_weights, thresholds_of

    from fractions import Fraction

    w = rank_weights([120.0, 40.0, 80.0])  # best .. worst: ranks 1, 3, 2
    assert [Fraction(x).limit_denominator(1000) for x in w] == [Fraction(1, 6), Fraction(3, 6), Fraction(2, 6)]
    assert rank_weights([5.0, 5.0, 1.0]) == [1 / 4, 1 / 4, 2 / 4]  # ties share the rank
    assert rank_weights([5.0, float("nan"), 1.0, None]) == [1 / 9, 3 / 9, 2 / 9, 3 / 9]  # no episode: the highest rank
    assert rank_weights([float("nan")] * 3) == [1 / 3] * 3 and rank_weights([7.0]) == [1.0]
    assert rank_weights([120.0, 40.0, 80.0], beta=0) == [1 / 3] * 3
    assert rank_weights([120.0, 40.0, 80.0], beta=2.0) == [1 / 14, 9 / 14, 4 / 14]
    assert rank_weights(np.array([[100.0, 20.0], [60.0, 60.0]]).mean(axis=1)) == [1 / 2, 1 / 2]
    for bad in (lambda: rank_weights([]), lambda: rank_weights([1.0], beta=-1)):
        with pytest.raises(ValueError):
            bad()
    # ---- set_weights on a pool built uniform, and back
    import torch

    pols = [DensePolicy(*PC.glorot(m, 96, *PP.SHAPES[m % 3]), device="cpu") for m in range(4)]
    pool = PartnerPool(pols)
    member = torch.full((8,), 255, dtype=torch.uint8)
    s = pool.struct_for(member)
    assert pool.thresholds is None and not s.thresholds and pool.thresholds_ref() is None
    pool.set_weights([1, 0, 2, 1])
    assert pool.thresholds == thresholds_of([1, 0, 2, 1]) == [2**30, 2**30, 3 * 2**30]
    assert [pool.thresholds_ref()[m] for m in range(3)] == pool.thresholds
    store = ctypes.addressof(pool.thresholds_ref().contents)
    pool.set_weights([0, 0, 0, 5])  # all weight on one member
    assert pool.thresholds == [0, 0, 0] == [pool.thresholds_ref()[m] for m in range(3)]
    assert ctypes.addressof(pool.thresholds_ref().contents) == store  # (one array for the pool's life: no pointer an env holds dangles)
    assert (PP.draws(9, 0, 0, 4096, 1.0, pool.thresholds)[1] == 3).all()
    s2 = pool.struct_for(member)
    assert [s2.thresholds[m] for m in range(3)] == [0, 0, 0]
    pool.set_weights(None)
    assert pool.thresholds is None and pool.thresholds_ref() is None and not pool.struct_for(member).thresholds
    weighted = PartnerPool(pols, weights=[1, 3, 0, 0])
    assert weighted.thresholds == thresholds_of([1, 3, 0, 0])
    weighted.set_weights(rank_weights([10.0, 30.0, 20.0, float("nan")]))
    assert weighted.thresholds == thresholds_of(rank_weights([10.0, 30.0, 20.0, float("nan")]))
    for bad in ([1, 2], [0, 0, 0, 0], [1, 1, 1, -1]):
        with pytest.raises(ValueError):
            pool.set_weights(bad)
    assert pool.thresholds is None  # (a refused call changes nothing)


def test_the_trajectory_row_defaults_keep_a_five_field_construction_working():
    from overcooked_ai_amd.trajectory_buffer import TrajectoryRow

    row = TrajectoryRow("r", "d", "a", "l", "s")
    assert row.ep_returns is None and row.member is None and tuple(row) == ("r", "d", "a", "l", "s", None, None)
    assert TrajectoryRow._fields == ("rewards", "done", "actions", "logp", "seat", "ep_returns", "member")
    rewards, done, actions, logp, seat = row[:5]
    assert (rewards, seat) == ("r", "s")
    assert TrajectoryRow("r", "d", "a", "l", None, "e")._replace(member="m").member == "m"
    from overcooked_ai_amd import trajectory_buffer as TB

    assert TB.RETURNS_ROW_BYTES == dict(ep_returns=16, member=1) and TB.RETURNS_ROW_ALIGN == dict(ep_returns=16, member=1)  # OcOutcomeBatch
    for name in TB.RETURNS_ROW_BYTES:
        offs = TB.row_offsets(name, 5, 130)
        assert offs == [t * 130 * TB.RETURNS_ROW_BYTES[name] for t in range(5)] and all(o % TB.RETURNS_ROW_ALIGN[name] == 0 for o in offs)
    assert TB.row_offsets("rewards", 3, 7) == [0, 112, 224]


def test_outcome_table_refuses_what_is_not_a_device_batch():
    import torch

    from overcooked_ai_amd.outcomes import Outcomes, outcome_table

    done, ep = torch.zeros((3, 5), dtype=torch.uint8), torch.zeros((3, 5, 4))
    seat = torch.zeros((3, 5), dtype=torch.uint8)
    for bad in (lambda: outcome_table(done, ep), lambda: outcome_table(done, ep[:, :, :3]), lambda: outcome_table(done.float(), ep),
                lambda: outcome_table(done, ep, member=seat, n_members=2), lambda: outcome_table(done, ep, seat=seat, member=seat),
                lambda: outcome_table(done, ep, seat=seat, member=seat, n_members=17), lambda: outcome_table(done, ep, seat=seat, n_members=2),
                lambda: outcome_table(done, ep, seat=seat[:2]), lambda: outcome_table(done[0], ep)):
        with pytest.raises(ValueError):
            bad()
    # ---- the host side of an Outcomes: one copy, the accessors on it
    t = OC.empty_table(8)
    t[0] = (2, 60, 2000, 20, 40, 7, 9, 30)
    t[1 + 2 * 1 + 0] = (1, 100, 10000, 100, 100, 3, 5, 60)  # member 1 plays seat 0
    t[7, 0] = 4
    out = Outcomes(torch.from_numpy(t), None, 3, True)
    assert (out.episodes, out.unattributed, out.min, out.max) == (3, 4, 20.0, 100.0) and out.mean == 160 / 3
    assert abs(out.std - np.std([20, 40, 100])) < 1e-12
    by = out.by_member()
    assert by["episodes"].shape == (3, 2) and by["episodes"][1, 0] == 1 and by["mean"][1, 0] == 100 and np.isnan(by["mean"][0, 0])
    assert by["min"][2, 1] == np.inf and by["max"][2, 1] == -np.inf and by["std"][1, 0] == 0
    none = Outcomes(torch.from_numpy(OC.empty_table(2)), None, 1, False)
    assert none.episodes == 0 and np.isnan(none.mean) and np.isnan(none.std)
    with pytest.raises(ValueError):
        none.by_member()
