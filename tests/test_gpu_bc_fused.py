"""oc_bc_epoch_fused on the device, held to oc_bc_update BIT FOR BIT through the C-ABI: every case of tests/bc_fused_cases.py runs
twice from identical initial weights, moments and clock — once through the staged chain, once through the fused kernel — and the
eight parameter arrays, the sixteen moment arrays, the clock, stats [K, 8] and info [K, 4] are compared as bit patterns (a NaN norm
in info compares as "a NaN", as in the Adam tests).  stats and info start as sentinels between guard rows that must come back untouched.

F1  every case: zero differing bits; what numpy says of the case (the count of kept rows of every minibatch, which minibatches are
    skipped) holds for both paths.
F2  the specials: a fully left-out minibatch in the middle is skipped, clock[3] counts it and the next one starts from untouched
    weights; NaN features in a left-out tile reach nothing (the zero-tile skip); a NaN feature in a kept row skips the minibatch
    in both paths and leaves weights and moments untouched; one minibatch more than a launch holds.
F3  a fused call repeats bit for bit; fused then staged equals staged then staged.
F4  BCLearner(fused=True): the 2 048-row, three-epoch run of tests/bc_cases.py with minibatches of 64, judged as tests/test_gpu_bc.py
    judges its run against the float64 restatement, then seated through dense_policy() and oc_partner_logits; the learner's scratch
    is not touched; a shape that is not served raises ValueError with the library's message."""
import ctypes

import numpy as np
import pytest
import torch

import bc_cases as BC
import bc_fused_cases as FC
from gpu_support import bits, guarded, guards_untouched, gpu, same  # noqa: F401

pytestmark = pytest.mark.gpu

FILL = FC.FILL
CLOCK0 = np.array([0.0, 1.0, 1.0, 0.0])


def same_info(x, y):
    """info rows: bit for bit, except that a NaN norm (column 0) compares as "a NaN" """
    nan = np.isnan(x[:, 0]) & np.isnan(y[:, 0])
    return same(np.where(nan, 0.0, x[:, 0]), np.where(nan, 0.0, y[:, 0])) and same(x[:, 1:], y[:, 1:])


class Epoch:
    """The device arrays of one case: inputs, parameters, moments, clock (fresh copies of the case's initial state), stats and info as
    sentinels between guard rows, and the staged path's scratch"""

    def __init__(self, c, dev):
        from overcooked_ai_amd.bc import scratch_rows

        feats, actions, index, cw, weights = FC.arrays_of(c)
        self.c, self.dev, self.dims, self.R = c, dev, (c.in_dim, c.h1, c.h2), len(actions)
        up = lambda x: torch.from_numpy(np.array(x)).to(dev)  # noqa: E731
        self.feats, self.actions, self.index = up(feats), up(actions), up(index)
        self.cw = up(cw) if cw is not None else None
        self.p = [up(w) for w in weights]
        self.m = [torch.zeros_like(t) for t in self.p]
        self.v = [torch.zeros_like(t) for t in self.p]
        self.clock = up(CLOCK0)
        self.K = len(FC.minibatches(c))
        self.new_outputs()
        rows, loss_rows, pol_rows, size = scratch_rows(c.n, c.M, *self.dims)
        f32 = dict(dtype=torch.float32, device=dev)
        self.scratch = [torch.empty((rows, 6), **f32), torch.empty((rows,), **f32), torch.empty((rows, 6), **f32), torch.empty((rows,), **f32),
                        torch.empty((loss_rows, 4), dtype=torch.float64, device=dev), torch.empty((pol_rows, size), **f32)]
        self.grads = [torch.empty_like(t) for t in self.p]

    def new_outputs(self):
        self.stats, self.g_stats = guarded(self.K, (8,), torch.float64, FILL, self.dev, before=2)
        self.info, self.g_info = guarded(self.K, (4,), torch.float64, FILL, self.dev, before=2)

    def _structs(self):
        from overcooked_ai_amd import _lib

        ptrs = ctypes.c_void_p * 8
        pol = _lib.OcActorCritic(*[t.data_ptr() for t in self.p], *self.dims)
        ad = _lib.OcAdam(ptrs(*[t.data_ptr() for t in self.m]), ptrs(*[t.data_ptr() for t in self.v]), self.clock.data_ptr(), None, None,
                         FC.HYPER["lr"], FC.HYPER["beta1"], FC.HYPER["beta2"], FC.HYPER["eps"], FC.CLIP if self.c.clip else 0.0)
        q = _lib.OcBcLoss(self.actions.data_ptr(), self.cw.data_ptr() if self.cw is not None else None, self.R, None, None, 0, 0, None, None, None, None, None)
        return pol, q, ad

    def run(self, fused):
        from overcooked_ai_amd import _lib

        c, L = self.c, _lib.load()
        pol, q, ad = self._structs()
        stream = torch.cuda.current_stream(self.dev).cuda_stream
        if fused:
            e = _lib.OcBcEpochFused(self.feats.data_ptr(), self.R, self.index.data_ptr(), c.n, c.M, self.stats.data_ptr(), self.info.data_ptr())
            rc = L.oc_bc_epoch_fused(ctypes.byref(pol), ctypes.byref(q), ctypes.byref(ad), ctypes.byref(e), stream)
        else:
            s = self.scratch
            u = _lib.OcBcUpdate(self.feats.data_ptr(), self.R, self.index.data_ptr(), c.n, c.M, s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(),
                                s[3].data_ptr(), s[4].data_ptr(), s[5].data_ptr(), _lib.OcPolicyGrads(*[t.data_ptr() for t in self.grads]),
                                self.stats.data_ptr(), self.info.data_ptr())
            rc = L.oc_bc_update(ctypes.byref(pol), ctypes.byref(q), ctypes.byref(ad), ctypes.byref(u), stream)
        assert rc == 0, L.oc_last_error().decode()
        torch.cuda.synchronize(self.dev)
        guards_untouched(c, "stats", self.g_stats, FILL)
        guards_untouched(c, "info", self.g_info, FILL)
        return self

    def results(self):
        host = lambda ts: np.concatenate([t.cpu().numpy().reshape(-1) for t in ts])  # noqa: E731
        return dict(parameters=host(self.p), first_moments=host(self.m), second_moments=host(self.v), clock=self.clock.cpu().numpy(),
                    stats=self.stats.cpu().numpy(), info=self.info.cpu().numpy())


def assert_same(x, y, what):
    for name in ("parameters", "first_moments", "second_moments", "clock", "stats"):
        differ = int((bits(x[name]) != bits(y[name])).sum())
        assert differ == 0, "%s: %d elements of the %s differ" % (what, differ, name)
    assert same_info(x["info"], y["info"]), "%s: info differs\n%s\n%s" % (what, x["info"], y["info"])


def both(c, dev):
    """(the staged path's results, the fused kernel's) from the case's initial state"""
    return Epoch(c, dev).run(False).results(), Epoch(c, dev).run(True).results()


def _special(name):
    return next(c for c in FC.CASES if c.special == name)


# ------------------------------------------------------------------------------------------ F1
@pytest.mark.parametrize("c", FC.CASES, ids=lambda c: c.id)
def test_f1_the_fused_epoch_equals_the_staged_one_bit_for_bit(c, gpu):
    staged, fused = both(c, gpu)
    assert_same(staged, fused, c.id)
    counts = FC.kept_counts(c)
    for r in (staged, fused):
        assert not (r["stats"] == FILL).any() and not (r["info"] == FILL).any()  # (every row written)
        assert r["stats"][:, 0].tolist() == counts
        skipped = r["info"][:, 3]
        assert all(skipped[k] == 1.0 for k, n in enumerate(counts) if n == 0)
        assert r["clock"][0] + r["clock"][3] == len(counts) and r["clock"][3] == skipped.sum()
        if c.clip and not c.special and c.h1 > 1:
            assert (r["info"][skipped == 0, 1] < 1.0).any(), "%s: no step was clipped" % c.id
    if not c.special:
        start = np.concatenate([w.reshape(-1) for w in FC.arrays_of(c)[4]])
        assert not same(fused["parameters"], start) and fused["clock"][0] >= 1


# ------------------------------------------------------------------------------------------ F2
def test_f2_a_fully_left_out_minibatch_in_the_middle_is_skipped(gpu):
    c = _special("middle_out")
    assert FC.kept_counts(c)[1] == 0 and FC.kept_counts(c)[0] > 0 and FC.kept_counts(c)[2] > 0
    staged, fused = both(c, gpu)
    assert_same(staged, fused, c.id)
    assert fused["info"][:, 3].tolist() == [0.0, 1.0, 0.0] and fused["clock"].tolist()[0] == 2.0 and fused["clock"][3] == 1.0
    assert not fused["stats"][1].any() and fused["info"][1, 0] == 0.0 and fused["info"][1, 2] == 0.0
    # the first minibatch alone leaves the weights from which the third starts: the skipped one moved nothing
    one = Epoch(c, gpu)
    one.c, one.K = c._replace(n=c.M), 1
    one.new_outputs()
    one.run(True)
    two = Epoch(c, gpu)
    two.c, two.K = c._replace(n=2 * c.M), 2
    two.new_outputs()
    two.run(True)
    for name in ("parameters", "first_moments", "second_moments"):
        assert same(one.results()[name], two.results()[name]), name
    assert not same(two.results()["parameters"], fused["parameters"])


def test_f2_nan_features_in_a_left_out_tile_reach_nothing(gpu):
    c = _special("nan_left_out")
    feats, actions, index, _, _ = FC.arrays_of(c)
    out = FC.left_out(c)
    assert np.isnan(feats[index[32:64]]).any() and out[32:64].all() and not out[:32].any()
    staged, fused = both(c, gpu)
    assert_same(staged, fused, c.id)
    for r in (staged, fused):
        assert all(np.isfinite(r[k]).all() for k in r) and r["info"][0, 3] == 0.0 and r["clock"][0] == 1.0 and r["stats"][0, 0] == 32


def test_f2_a_nan_feature_in_a_kept_row_skips_the_minibatch_in_both_paths(gpu):
    c = _special("nan_kept")
    staged, fused = both(c, gpu)
    assert_same(staged, fused, c.id)
    for r in (staged, fused):
        assert np.isnan(r["info"][1, 0]) and r["info"][:, 3].tolist() == [0.0, 1.0, 0.0] and r["clock"][0] == 2.0 and r["clock"][3] == 1.0
        assert np.isfinite(r["parameters"]).all() and np.isfinite(r["first_moments"]).all() and np.isfinite(r["second_moments"]).all()
    one = Epoch(c, gpu)
    one.c, one.K = c._replace(n=c.M), 1
    one.new_outputs()
    two = Epoch(c, gpu)
    two.c, two.K = c._replace(n=2 * c.M), 2
    two.new_outputs()
    a, b = one.run(True).results(), two.run(True).results()
    for name in ("parameters", "first_moments", "second_moments"):  # untouched by the skipped minibatch, by bit pattern
        assert same(a[name], b[name]), name


def test_f2_one_minibatch_more_than_a_launch_holds(gpu):
    from overcooked_ai_amd.bc import plan_bc_epoch_fused

    c = _special("chain")
    assert c.n == FC.per_launch() + 1 and c.M == 1 and "2 launch(es)" in plan_bc_epoch_fused(c.n, c.M, c.in_dim, c.h1, c.h2)
    staged, fused = both(c, gpu)
    assert_same(staged, fused, c.id)
    assert fused["stats"][-1, 0] == FC.kept_counts(c)[-1] and fused["clock"][0] == sum(FC.kept_counts(c))


# ------------------------------------------------------------------------------------------ F3
def test_f3_a_fused_call_repeats_bit_for_bit_and_alternates_with_the_staged_path(gpu):
    c = next(c for c in FC.CASES if c.n == 150 and c.in_dim == 96 and c.h1 == 64)
    again, fused = Epoch(c, gpu).run(True).results(), Epoch(c, gpu).run(True).results()
    assert_same(again, fused, c.id + " twice")
    mixed, staged = Epoch(c, gpu).run(True), Epoch(c, gpu).run(False)
    for e in (mixed, staged):  # a second, staged epoch from the state the first left
        e.new_outputs()
        e.run(False)
    assert_same(staged.results(), mixed.results(), c.id + " fused then staged")
    assert staged.results()["clock"][0] == 6.0


# ------------------------------------------------------------------------------------------ F4
def test_f4_the_small_run_learns_with_fused_minibatches_of_64(gpu):
    """tests/test_gpu_bc.py's run (2 048 rows, three epochs, the reference's permutations and initial weights) with minibatches of 64
    through the fused kernel, judged by that test's criterion: the last minibatch's loss below the midpoint of the float64 run's first
    and last losses, evaluate()'s accuracy above the midpoint of its initial and final accuracies; the first minibatch's loss within
    1e-5 of the float64 restatement on the same weights and rows."""
    from overcooked_ai_amd import _lib
    from overcooked_ai_amd.bc import BCLearner
    from overcooked_ai_amd.policy import ActorCritic
    import policy_cases as PC

    e = BC.E2E
    feats_h, actions_h, student, perms = BC.e2e_inputs()
    losses64, acc0, acc1 = BC.e2e_reference()
    feats, actions = torch.from_numpy(feats_h.copy()).to(gpu), torch.from_numpy(actions_h.copy()).to(gpu)
    policy = ActorCritic.from_weights(*student, device=gpu)
    learner = BCLearner(policy, lr=e.lr)
    got = []
    for perm in perms:
        stats, info = learner.epoch(feats, actions, torch.from_numpy(perm.copy()).to(gpu), 64, fused=True)
        assert stats.shape == (e.rows // 64, 8) and info.shape == (e.rows // 64, 4) and not bool(info[:, 3].any())
        got += stats[:, 1].tolist()
    assert learner._scratch == {}  # (no scratch was allocated)
    after = learner.evaluate(feats, actions)
    first = BC._f64_eval(student, feats_h[perms[0][:64]], actions_h[perms[0][:64]]).stats[1]
    print("loss %.4f -> %.4f on the device (fused, minibatch 64), %.4f -> %.4f in float64 (minibatch 256); accuracy -> %.4f, %.4f -> %.4f in float64"
          % (got[0], got[-1], losses64[0], losses64[-1], float(after.accuracy), acc0, acc1))
    assert float(learner.adam.clock[0]) == len(got) == 3 * e.rows // 64
    assert abs(got[0] - first) <= 1e-5 * first  # (the first minibatch: the same weights on both sides)
    assert got[-1] < 0.5 * (losses64[0] + losses64[-1])
    assert float(after.accuracy) > 0.5 * (acc0 + acc1)
    # ---- the staged path from the same start gives the same weights, and the optimiser's state is shared
    twin = ActorCritic.from_weights(*student, device=gpu)
    staged = BCLearner(twin, lr=e.lr)
    for perm in perms:
        staged.epoch(feats, actions, torch.from_numpy(perm.copy()).to(gpu), 64)
    assert all(torch.equal(p, q) for p, q in zip(policy._params(), twin._params()))
    assert torch.equal(learner.adam.clock, staged.adam.clock) and all(torch.equal(x, y) for x, y in zip(learner.adam.m + learner.adam.v, staged.adam.m + staged.adam.v))
    # ---- the trained policy as a partner
    n = 300
    dense = policy.dense_policy()
    seat = torch.full((n,), 7, dtype=torch.uint8, device=gpu)
    theirs = torch.full((n, 2, 6), FILL, dtype=torch.float32, device=gpu)
    seats = _lib.OcPartnerSeats(seat.data_ptr(), None, 1.0, 12345, 3, 8)
    b = _lib.OcBatch(n_envs=n)
    L = _lib.load()
    rc = L.oc_partner_logits(ctypes.byref(b), dense._ref, ctypes.byref(seats), feats.data_ptr(), (e.in_dim - 56) // 20, theirs.data_ptr(),
                             torch.cuda.current_stream(gpu).cuda_stream)
    assert rc == 0, L.oc_last_error().decode()
    with torch.no_grad():
        mine, _ = policy(feats[:2 * n].contiguous())
    seat, theirs, mine = seat.cpu().numpy(), theirs.cpu().numpy(), mine.cpu().numpy().reshape(n, 2, 6)
    env = np.arange(n)
    assert (seat <= 1).all() and same(theirs[env, seat], mine[env, seat])
    assert not same(mine, PC.forward_f64(feats_h[:2 * n], student)[2][:, :6].astype(np.float32).reshape(n, 2, 6))  # (the weights moved)


def test_f4_the_learner_refuses_what_the_fused_kernel_does_not_serve(gpu):
    from overcooked_ai_amd.bc import BCLearner
    from overcooked_ai_amd.policy import ActorCritic

    feats = torch.zeros((300, 96), device=gpu)
    acts = torch.zeros(300, dtype=torch.uint8, device=gpu)
    index = torch.arange(258, dtype=torch.int32, device=gpu)
    learner = BCLearner(ActorCritic(96, 64, 64, seed=1).to(gpu))
    with pytest.raises(ValueError, match="oc_bc_epoch_fused: minibatch must be in 1..128"):
        learner.epoch(feats, acts, index, 129, fused=True)
    with pytest.raises(ValueError, match="oc_bc_epoch_fused: minibatch must be in 1..128"):
        learner.update(feats, acts, index[:129], fused=True)
    stats, info = learner.update(feats, acts, index[:128], fused=True)
    assert stats.shape == (1, 8) and float(stats[0, 0]) == 128 and learner._scratch == {}
    stats, info = learner.epoch(feats, acts, index, 129)  # (the staged path serves it)
    assert stats.shape == (2, 8) and list(learner._scratch) == [129]
