"""oc_policy_backward on the device, held BIT FOR BIT to the header's backward arithmetic restated in numpy (tests/backward_chain.py;
include/oc_amd.h: OcActorCritic "Backward arithmetic"): the delta chains from +0, the ReLU derivative by the f32 pre-activation, the
dealing of 32-row tiles to wavefronts and workgroups, ONE f32 accumulator per element and wavefront over its tiles and their rows in
ascending order — fmaf for the weights, addition for the biases —, ((w0 + w1) + w2) + w3 into the workgroup's partial, the partials
in ascending order, all-zero tiles skipped.  B1 of tests/test_gpu_policy.py holds for any float32 order of summation and E1-E3 are
exact in every order; these comparisons are equalities (after -0 -> +0; no accumulator is ever -0), and
tests/test_host_backward_chain.py shows on the CPU that numpy's own float32 order and eleven restatements that each change one
sentence fail them.  The calls are tests/backward_chain_cases.py's, through test_gpu_policy's `backward`: inputs at the header's
minimum alignments, sentinel-filled outputs between guard rows, partials of exactly the planned G rows.

H1  every float of every one of the G partials and every element of the eight gradients of every case is the restatement's; the
    gradients are the device's own partials added in ascending order; the guards and the rows behind the G-th partial are untouched.
    The first array, element and owner workgroup that differ are named with both bit patterns.
H2  at 116 and 136 inputs the rows 96.. of gw1, which a second launch accumulates, are the restatement's too, and not zeros.
H3  a sparse multi-pass call repeats bit for bit; its first two passes as a call of their own (2 * one_pass rows: every tile keeps
    its wavefront and workgroup) and its rows behind them as another (three workgroups, the owners again the same) each give their
    own restatement's partials and their own partials' sum.  (The whole call is NOT the float32 sum of the two: a wavefront's
    accumulator goes on from its second tile to its third by fmaf, which no addition of two partials restates.)
H4  the two NaN-filled cases — NaN in the feature rows of every all-zero tile — give finite gradients, the bits of the cases without.
H5  one link downstream: oc_policy_forward on a 257-row case, oc_ppo_loss on a batch of tests/ppo_loss_cases.py over those logits and
    values, then oc_policy_backward on the device's own d_grad_logits and d_grad_values as they were read back — the gradients a
    training run feeds it, one tile of them all the partner's zeros — against the restatement evaluated on the arrays read back.

Every test prints how many partial floats and gradient elements it compared, and the running total."""
import types

import numpy as np
import pytest

import backward_chain as BC
import backward_chain_cases as CC
import mlp_chain as MC
import policy_cases as PC
import ppo_loss_cases as LC

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from gpu_support import bits, gpu  # noqa: E402, F401
from test_gpu_policy import backward, forward  # noqa: E402
from test_gpu_ppo_loss import run as ppo_loss  # noqa: E402

COMPARED = {"partial floats": 0, "gradient elements": 0}
_DEVICE = {}


def device_of(c, dev):
    """(the eight gradient arrays, the partials) of the case's call on the device, once per case"""
    if c.id not in _DEVICE:
        _DEVICE[c.id] = backward(c, CC.arrays_of(c), dev)
    return _DEVICE[c.id]


def first_difference(c, got, want):
    """Words for the first element (in the layout's order) at which float32 [size] got and want differ in their bits, or None"""
    g, w = MC.canon(got), MC.canon(want)
    for name, where in PC.layout_of(c).items():
        at = np.flatnonzero(g[where] != w[where])
        if at.size:
            i = at[0]
            return "%s: %d of %d elements differ, the first [%d]: %r (0x%08X), not %r (0x%08X)" % (
                name, at.size, g[where].size, i, float(got[where][i]), int(g[where][i]), float(want[where][i]), int(w[where][i]))
    return None


def held(c, grads, partials, ref):
    """The device's partials and gradients of a call of case c's shape are the Restated ref's, bit for bit"""
    grid, waves = ref.partials.shape[0], PC.backward_plan_of(c)[1]
    assert ref.smallest >= MC.MIN_NORMAL, (c.id, ref.smallest)
    assert partials.shape == ref.partials.shape and partials.dtype == np.float32, (c.id, partials.shape, ref.partials.shape)
    group, _ = BC.owner_of_tiles(ref.live, grid, waves)
    wrong = np.flatnonzero((MC.canon(partials) != MC.canon(ref.partials)).any(1))
    if wrong.size:
        p = int(wrong[0])
        pytest.fail("%s: %d of the %d partials are not the restatement's; the first, of workgroup %d (%d wavefronts; live tiles %s): %s"
                    % (c.id, wrong.size, grid, p, waves, ref.live[group == p].tolist(), first_difference(c, partials[p], ref.partials[p])))
    got = BC.flat(grads)
    said = first_difference(c, got, BC.add_partials(partials))
    assert said is None, "%s: the gradients are not the device's own %d partials added in ascending order: %s" % (c.id, grid, said)
    said = first_difference(c, got, BC.flat(ref.grads))
    assert said is None, "%s: the gradients are not the restatement's: %s" % (c.id, said)
    assert [g.shape for g in grads] == [g.shape for g in ref.grads]
    COMPARED["partial floats"] += partials.size
    COMPARED["gradient elements"] += got.size
    print("%s: %d partial floats (%d partials, %d live tiles) and %d gradient elements compared bit for bit (so far %d and %d)"
          % (c.id, partials.size, grid, len(ref.live), got.size, COMPARED["partial floats"], COMPARED["gradient elements"]))


@pytest.mark.parametrize("c", CC.CASES, ids=lambda c: c.id)
def test_h1_every_partial_and_gradient_is_the_restatement_s_bit_for_bit(c, gpu):
    ref = CC.restated_of(c, watch=True)
    grads, partials = device_of(c, gpu)
    assert partials.shape[0] == PC.backward_plan_of(c)[0]
    held(c, grads, partials, ref)


@pytest.mark.parametrize("c", [c for c in CC.CASES if c.in_dim > 96], ids=lambda c: c.id)
def test_h2_the_second_launch_keeps_the_order_of_summation(c, gpu):
    ref = CC.restated_of(c, watch=True)
    grads, partials = device_of(c, gpu)
    behind = slice(96 * c.h1, c.in_dim * c.h1)  # rows 96.. of gw1 in a partial
    assert np.array_equal(MC.canon(partials[:, behind]), MC.canon(ref.partials[:, behind])), c.id
    assert np.array_equal(MC.canon(grads[0][96:]), MC.canon(ref.grads[0][96:])) and grads[0][96:].shape == (c.in_dim - 96, c.h1), c.id
    assert (grads[0][96:] != 0).mean() > 0.5, c.id
    COMPARED["partial floats"] += partials[:, behind].size
    COMPARED["gradient elements"] += grads[0][96:].size


def same(x, y):
    return all(np.array_equal(bits(p), bits(q)) for p, q in zip(x[0] + [x[1]], y[0] + [y[1]]))


def test_h3_a_sparse_multi_pass_call_repeats_and_its_passes_alone_are_their_own_restatements(gpu):
    c = CC.named("96_64_64-%drows-contiguous-sparse" % PC.three_passes(96))
    a = CC.arrays_of(c)
    whole = device_of(c, gpu)
    assert same(whole, backward(c, a, gpu)), c.id  # a call repeats bit for bit
    grid, waves = PC.backward_plan_of(c)
    cut = 2 * PC.one_pass(c.in_dim)
    assert cut % (32 * waves * grid) == 0  # no tile is cut, and every tile on either side keeps its wavefront and workgroup
    x, d3 = PC.rows_of(a), PC.upstream(a)
    for lo, hi in ((0, cut), (cut, c.M)):
        part = c._replace(id="%s rows %d..%d" % (c.id, lo, hi), M=hi - lo)
        g, w = PC.backward_plan_of(part)
        assert w == waves and g == min(grid, -(-(hi - lo) // (32 * waves)))
        ref = BC.restate(x[lo:hi], d3[lo:hi], a.weights, g, w, watch=True)
        tiles = CC.listed_tiles(c)
        tiles = tiles[(tiles >= lo // 32) & (tiles < -(-hi // 32))]
        assert np.array_equal(ref.live, tiles - lo // 32)
        for mine, theirs in zip(BC.owner_of_tiles(ref.live, g, w), BC.owner_of_tiles(tiles, grid, waves)):
            assert np.array_equal(mine, theirs)
        grads, partials = backward(c, a, gpu, lo=lo, n_rows=hi - lo)
        held(part, grads, partials, ref)
        assert all(np.abs(q).max() > 0 for q in grads), part.id


@pytest.mark.parametrize("c", CC.NAN, ids=lambda c: c.id)
def test_h4_nan_in_the_features_of_skipped_tiles_changes_no_bit(c, gpu):
    a = CC.arrays_of(c)
    dead = ~np.isin(np.arange(c.M) // 32, CC.listed_tiles(c))
    assert np.isnan(a.features[a.rows[dead]]).all() and np.isfinite(a.features[a.rows[~dead]]).all() and dead.sum() > c.M - 42 * 32
    grads, partials = device_of(c, gpu)
    assert all(np.isfinite(g).all() for g in grads) and np.isfinite(partials).all(), c.id
    held(c, grads, partials, CC.restated_of(c, watch=True))
    assert same((grads, partials), device_of(CC.base_of(c), gpu)), c.id


LOSS_CASE = next(c for c in LC.CASES if c.M == 257 and c.mode == "indexed" and c.seat == "all0")
PARTNER_TILE = slice(160, 192)  # the rows of the call that are made the partner's samples, all 32 of them (no env has both its players there)


def loss_batch():
    """The arrays of LOSS_CASE with the seats of the samples of rows 160..191 turned so that these are the partner's"""
    a = LC.arrays_of(LOSS_CASE)
    seat = a.seat.copy()
    s = a.sample[PARTNER_TILE]
    s = s[(s >= 0) & (s < a.S)]
    seat[s >> 1] = s & 1  # a sample is the partner's where seat[env] == player
    b = types.SimpleNamespace(**vars(a))
    b.seat = seat
    partner = np.array([not 0 <= s < a.S or seat[s >> 1] == (s & 1) for s in a.sample])
    assert partner[PARTNER_TILE].all() and 0.3 < partner.mean() < 0.7, "two rows of the tile are one env's two players"
    return b, partner


def test_h5_backward_on_the_gradients_oc_ppo_loss_wrote(gpu):
    c = CC.named("96_64_64-257rows-indexed-dense")
    a = CC.arrays_of(c)
    out = forward(c, a, gpu)
    batch, partner = loss_batch()
    batch.logits, batch.values = np.ascontiguousarray(out[:, :6]), np.ascontiguousarray(out[:, 6])
    loss = ppo_loss(LOSS_CASE, batch, gpu)
    # ---- the device's own d_grad_logits and d_grad_values, as read back
    fed = a._replace(grad_logits=loss.grad_logits, grad_values=loss.grad_values)
    d3 = PC.upstream(fed)
    left_out = LC.loss_f64(LOSS_CASE, batch).left_out  # the partner's samples, the sampler's invalid rows, entries outside the batch
    raw = CC.raw_upstream(fed)
    assert partner[PARTNER_TILE].all() and left_out[partner].all() and not bits(raw[left_out]).any()  # +0 by bit pattern
    assert (raw[~left_out] != 0).any(1).mean() > 0.5 and np.isfinite(raw).all()
    grid, waves = PC.backward_plan_of(c)
    ref = BC.restate(PC.rows_of(fed), d3, a.weights, grid, waves, watch=True)
    assert 5 not in ref.live.tolist() and len(ref.live) >= 7 and (~a.valid & (raw != 0).any(1)).any()
    grads, partials = backward(c, fed, gpu)
    held(c._replace(id=c.id + " on oc_ppo_loss's gradients"), grads, partials, ref)
    assert all(np.abs(g).max() > 0 for g in grads)
