"""oc_adam_step and oc_ppo_update on the device, through the C-ABI on arrays at the header's minimum alignments between guard bytes,
and through `learner.Adam` / `learner.PPOLearner`.

G1  every case, every step: parameters, moments, clock and info equal tests/learner_cases.py's restatement as BIT PATTERNS (a NaN
    norm: a NaN); guard bytes untouched; gradients unchanged.
G2  skipped steps (NaN, +inf, scale 0): parameters, moments, steps and powers bit-unchanged, skipped incremented, and the next good
    step is the step from the state before the skipped one.
G3  a call repeats bit for bit from the same state.
G4  learner.Adam.step() after loss.backward() against clip_grad_norm_ + torch.optim.Adam on cloned parameters, five steps, within
    4 x F32_ERROR.
G5  oc_ppo_update with K = 1 = forward, loss, backward on the raw gradients, oc_adam_step with the stats' 1 / count, bit for bit.
G6  an epoch of K = 3 with a shorter last minibatch = three K = 1 calls, bit for bit, and repeats bit for bit.
G7  one PPOLearner.update held link by link to the float64 chain: forward, loss, backward, and the parameter change against the
    float64 Adam within learner_cases.update_bound.
G8  a collected buffer end to end; every minibatch's stats are ppo_loss's on the weights held at that point; the value loss of a
    fixed minibatch falls over 10 updates, as it does in float64.
Observed on an MI355X: G1 bit for bit in all 96 steps; G4 largest error / (4 x F32_ERROR) 0.102; G7 largest |device step - float64
step| / bound 0.0148 (profiles/learner.txt)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import learner_cases as LC
import policy_cases as PC
import ppo_loss_cases as PL
from gpu_support import Fenced, bits, gpu, same  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = LC.DEVICE_FACTOR * LC.F32_ERROR


class Optimiser:
    """The device state of one oc_adam_step caller: parameters, moments, clock, info, gradients, each Fenced"""

    def __init__(self, dims, params, dev, m=None, v=None, clock=None):
        self.dims, self.dev = dims, dev
        zeros = [np.zeros(s, np.float32) for s in LC.shapes(*dims)]
        self.p = [Fenced(a, 4, dev) for a in params]
        self.m = [Fenced(a, 4, dev) for a in (zeros if m is None else m)]
        self.v = [Fenced(a, 4, dev) for a in (zeros if v is None else v)]
        self.g = [Fenced(a, 4, dev) for a in zeros]
        self.clock = Fenced(LC.CLOCK0 if clock is None else clock, 8, dev)
        self.info = Fenced(np.full(4, LC.FILL), 8, dev)
        self.scale = Fenced(np.zeros(1), 8, dev)

    def structs(self, hyper, scaled):
        from overcooked_ai_amd import _lib

        ptrs = ctypes.c_void_p * 8
        pol = _lib.OcActorCritic(*[f.ptr for f in self.p], *self.dims)
        grads = _lib.OcPolicyGrads(*[f.ptr for f in self.g])
        ad = _lib.OcAdam(ptrs(*[f.ptr for f in self.m]), ptrs(*[f.ptr for f in self.v]), self.clock.ptr, self.scale.ptr if scaled else None,
                         self.info.ptr, hyper.lr, hyper.beta1, hyper.beta2, hyper.eps, hyper.max_grad_norm if hyper.max_grad_norm is not None else 0.0)
        return pol, grads, ad

    def step(self, hyper, grads, scale=None):
        from overcooked_ai_amd import _lib

        for f, a in zip(self.g, grads):
            f.t.copy_(torch.from_numpy(np.array(a, np.float32)))  # (a copy of the bytes: a NaN arrives as it is)
        if scale is not None:
            self.scale.t.fill_(scale)
        pol, gr, ad = self.structs(hyper, scale is not None)
        L = _lib.load()
        rc = L.oc_adam_step(ctypes.byref(pol), ctypes.byref(gr), ctypes.byref(ad), torch.cuda.current_stream(self.dev).cuda_stream)
        assert rc == 0, L.oc_last_error().decode()
        torch.cuda.synchronize(self.dev)

    def state(self):
        return LC.State(LC.flat([f.host() for f in self.p]), LC.flat([f.host() for f in self.m]), LC.flat([f.host() for f in self.v]), self.clock.host())

    def intact(self):
        return all(f.intact() for f in self.p + self.m + self.v + self.g + [self.clock, self.info, self.scale])


def assert_state(got, want, what):
    for name, x, y in zip(("parameters", "first moments", "second moments", "clock"), got, want):
        assert same(x, y), "%s: the %s differ in %d elements" % (what, name, int((bits(x) != bits(y)).sum()))


def assert_info(got, want, what):
    if np.isnan(want[0]):
        assert np.isnan(got[0]) and same(got[1:], want[1:]), (what, got, want)
    else:
        assert same(got, want), (what, got, want)


# ------------------------------------------------------------------------------------------ G1-G3: oc_adam_step
@pytest.mark.parametrize("c", LC.CASES, ids=lambda c: c.id)
def test_g1_every_step_equals_the_restatement_bit_for_bit(c, gpu):
    params, steps = LC.inputs_of(c)
    opt = Optimiser((c.in_dim, c.h1, c.h2), params, gpu)
    for t, (st, (want, info)) in enumerate(zip(steps, LC.trajectory_of(c))):
        what = "%s step %d" % (c.id, t)
        opt.step(c.hyper, st.grads, st.scale)
        assert_state(opt.state(), want, what)
        assert_info(opt.info.host(), info, what)
        assert opt.intact(), what + ": guard bytes written"
        assert all(same(f.host(), g) for f, g in zip(opt.g, st.grads)), what + ": gradients changed"


@pytest.mark.parametrize("pattern", ("nan", "inf", "scale0"))
def test_g2_a_skipped_step_writes_nothing_and_the_next_continues(pattern, gpu):
    for c in (c for c in LC.CASES if c.pattern == pattern):
        params, steps = LC.inputs_of(c)
        opt = Optimiser((c.in_dim, c.h1, c.h2), params, gpu)
        opt.step(c.hyper, steps[0].grads, steps[0].scale)
        before = opt.state()
        opt.step(c.hyper, steps[1].grads, steps[1].scale)
        after, info = opt.state(), opt.info.host()
        assert all(same(x, y) for x, y in zip(before[:3], after[:3])) and same(before.clock[:3], after.clock[:3]), c.id
        assert before.clock[3] == 0.0 and after.clock[3] == 1.0 and info[3] == 1.0 and info[1] == 0.0, c.id
        opt.step(c.hyper, steps[2].grads, steps[2].scale)
        direct, _ = LC.adam_f32(before, steps[2].grads, c.hyper, steps[2].scale)  # as if the skipped step had not been made
        got = opt.state()
        assert_state(got[:3], direct[:3], c.id)
        assert same(got.clock[:3], direct.clock[:3]) and got.clock[3] == 1.0 and opt.info.host()[3] == 0.0 and opt.intact(), c.id


def test_g3_a_call_repeats_bit_for_bit(gpu):
    for c in (c for c in LC.CASES if c.pattern in ("above", "scale_count", "nan")):
        params, steps = LC.inputs_of(c)
        (first, _), = LC.trajectory_of(c)[:1]
        dims = (c.in_dim, c.h1, c.h2)
        results = []
        for _ in range(2):  # twice from the state behind the first step: carried moments and clock
            opt = Optimiser(dims, LC.split(first.params, *dims), gpu, LC.split(first.m, *dims), LC.split(first.v, *dims), first.clock)
            opt.step(c.hyper, steps[1].grads, steps[1].scale)
            results.append((opt.state(), opt.info.host()))
        assert_state(results[0][0], results[1][0], c.id)
        assert same(results[0][1], results[1][1]), c.id  # (the same call: the same NaN too)


# ------------------------------------------------------------------------------------------ G4: learner.Adam
def test_g4_adam_step_against_torch_s_pair_on_cloned_parameters(gpu):
    from overcooked_ai_amd.learner import Adam
    from overcooked_ai_amd.policy import ActorCritic

    c = next(c for c in PC.CASES if c.id.endswith("96_64_64-257rows-indexed-dense"))
    a = PC.arrays_of(c)
    w = lambda x: float(np.float32(x))  # noqa: E731  (torch is given the float32 hyperparameters the C call takes: test_host_learner.py)
    for max_norm, lr in ((0.1, 1e-3), (None, 5e-5), (50.0, 1e-3)):
        policy = ActorCritic.from_weights(*a.weights, device=gpu)
        twin = [torch.nn.Parameter(p.detach().clone()) for p in policy._params()]
        theirs = torch.optim.Adam(twin, lr=w(lr), betas=(w(0.9), w(0.999)), eps=w(1e-8))
        mine = Adam(policy, lr=lr, max_grad_norm=max_norm)
        feats, index = torch.from_numpy(a.features.copy()).to(gpu), torch.from_numpy(a.index.copy()).to(gpu)
        gl, gv = torch.from_numpy(a.grad_logits.copy()).to(gpu), torch.from_numpy(a.grad_values.copy()).to(gpu)
        before = [p.data_ptr() for p in policy._params()]
        worst = 0.0
        for t in range(5):
            mine.zero_grad()
            logits, values = policy(feats, index)
            ((logits * gl).sum() * (1.0 + t) + (values * gv).sum()).backward()
            for q, p in zip(twin, policy._params()):
                q.grad = p.grad.detach().clone()
            if max_norm is not None:
                norm = torch.nn.utils.clip_grad_norm_(twin, w(max_norm))
            theirs.step()
            mine.step()
            assert float(mine.info[3]) == 0.0 and float(mine.clock[0]) == t + 1
            if max_norm is not None:
                assert abs(float(mine.info[0]) - float(norm)) <= 1e-5 * float(norm)
            got = LC.State(*(LC.flat([x.detach().cpu().numpy() for x in xs]) for xs in (policy._params(), mine.m, mine.v)), None)
            ref = LC.State(LC.flat([q.detach().cpu().numpy() for q in twin]), LC.flat([theirs.state[q]["exp_avg"].cpu().numpy() for q in twin]),
                           LC.flat([theirs.state[q]["exp_avg_sq"].cpu().numpy() for q in twin]), None)
            worst = max(worst, LC.state_error(got, ref))
        print("max_grad_norm %r: largest error against torch over 5 steps / (4 * F32_ERROR) %.3g" % (max_norm, worst / TOL))
        assert worst <= TOL and before == [p.data_ptr() for p in policy._params()]
        assert LC.rel(got.params, LC.flat(a.weights)) > 100 * LC.F32_ERROR  # (the steps moved the parameters)
        # the state travels: a second optimiser that loads it makes the same next step
        again = Adam(policy, lr=lr, max_grad_norm=max_norm)
        again.load_state_dict(mine.state_dict())
        assert torch.equal(again.clock, mine.clock) and all(torch.equal(x, y) for x, y in zip(again.m + again.v, mine.m + mine.v))


# ------------------------------------------------------------------------------------------ G5, G6: oc_ppo_update
HYPER = LC.Hyper(1e-3, 0.9, 0.999, 1e-8, 0.1)
LOSS = (0.05, 10.0, 0.5, 0.1, 0.0)  # clip_param, vf_clip_param, vf_loss_coeff, entropy_coeff, kl_coeff


def _batch_arrays(S, seed, seat):
    rng = np.random.default_rng(seed)
    actions = rng.integers(0, 6, S).astype(np.uint8)
    actions[rng.random(S) < 0.03] = 255
    seats = {None: None, "mixed": rng.choice(np.array([0, 1, 255], np.uint8), size=S // 2), "all0": np.zeros(S // 2, np.uint8)}[seat]
    return types.SimpleNamespace(S=S, actions=actions, logp_old=rng.normal(-1.8, 0.3, S).astype(np.float32),
                                 advantages=(0.3 + 1.5 * rng.standard_normal(S)).astype(np.float32),
                                 targets=(3 * rng.standard_normal(S)).astype(np.float32), seat=seats, logits_old=None, moments=None)


class Update:
    """The device arrays of oc_ppo_update calls on one policy case: features, batch side, index, scratch, and an Optimiser"""

    def __init__(self, c, dev, seat, index=None, partner_only=False, K=1):
        from overcooked_ai_amd.learner import scratch_rows

        a = PC.arrays_of(c)
        self.c, self.dev, self.dims = c, dev, (c.in_dim, c.h1, c.h2)
        R = len(a.features)
        S = R + (R & 1)
        feats = np.concatenate([a.features, np.zeros((S - R, c.in_dim), np.float32)])
        index = (a.index if index is None else index).copy()
        if partner_only:  # player 0's samples under seats that make every one of them the partner's
            index = (2 * (np.abs(index.astype(np.int64)) % (S // 2))).astype(np.int32)
        self.index_host, self.feats_host = index, feats
        self.batch_host = b = _batch_arrays(S, c.seed, seat)
        self.feats, self.index = Fenced(feats, 16, dev), Fenced(index, 4, dev)
        self.batch = [Fenced(x, al, dev) if x is not None else None for x, al in ((b.actions, 1), (b.logp_old, 4), (b.advantages, 4), (b.targets, 4), (b.seat, 1))]
        self.M = M = -(-len(index) // K)
        rows, loss_rows, pol_rows, size = scratch_rows(len(index), M, *self.dims)
        f32 = np.float32
        self.logits, self.values = Fenced(np.full((rows, 6), LC.FILL, f32), 16, dev), Fenced(np.full(rows, LC.FILL, f32), 4, dev)
        self.gl, self.gv = Fenced(np.full((rows, 6), LC.FILL, f32), 16, dev), Fenced(np.full(rows, LC.FILL, f32), 4, dev)
        self.lp, self.pp = Fenced(np.full((loss_rows, 6), LC.FILL), 8, dev), Fenced(np.full((pol_rows, size), LC.FILL, f32), 4, dev)
        self.opt = Optimiser(self.dims, a.weights, dev)
        self.n_stats = -(-len(index) // M)
        self.stats, self.info = Fenced(np.full((self.n_stats, 8), LC.FILL), 8, dev), Fenced(np.full((self.n_stats, 4), LC.FILL), 8, dev)

    def loss_struct(self, **kw):
        from overcooked_ai_amd import _lib

        p = lambda f: f.ptr if f is not None else None  # noqa: E731
        v = dict(d_logits=None, d_values=None, d_index=None, n_minibatch=0, d_grad_logits=None, d_grad_values=None, d_partials=None, d_stats=None)
        v.update(kw)
        return _lib.OcPpoLoss(p(self.batch[0]), p(self.batch[1]), p(self.batch[2]), p(self.batch[3]), p(self.batch[4]), None, None, self.batch_host.S,
                              v["d_logits"], v["d_values"], v["d_index"], 0, v["n_minibatch"], v["d_grad_logits"], v["d_grad_values"], v["d_partials"],
                              v["d_stats"], None, *LOSS)

    def update(self, lo=0, n=None, M=None, k0=0):
        """oc_ppo_update on index entries lo .. lo + n - 1 in minibatches of M, stats and info from row k0 on"""
        from overcooked_ai_amd import _lib

        n = len(self.index_host) - lo if n is None else n
        pol, grads, ad = self.opt.structs(HYPER, False)
        u = _lib.OcPpoUpdate(self.feats.ptr, len(self.feats_host), self.index.ptr + 4 * lo, n, self.M if M is None else M, self.logits.ptr, self.values.ptr,
                             self.gl.ptr, self.gv.ptr, self.lp.ptr, self.pp.ptr, grads, self.stats.ptr + 64 * k0, self.info.ptr + 32 * k0)
        q = self.loss_struct()
        L = _lib.load()
        rc = L.oc_ppo_update(ctypes.byref(pol), ctypes.byref(q), ctypes.byref(ad), ctypes.byref(u), torch.cuda.current_stream(self.dev).cuda_stream)
        assert rc == 0, L.oc_last_error().decode()
        torch.cuda.synchronize(self.dev)

    def four_calls(self):
        """The same minibatch (the whole index) by the four entry points one by one, with the same scratch"""
        from overcooked_ai_amd import _lib

        n = len(self.index_host)
        pol, grads, ad = self.opt.structs(HYPER, False)
        ad.d_grad_scale, ad.d_info = self.stats.ptr + 56, self.info.ptr
        rows = _lib.OcPolicyRows(self.feats.ptr, len(self.feats_host), self.index.ptr, 0, n)
        q = self.loss_struct(d_logits=self.logits.ptr, d_values=self.values.ptr, d_index=self.index.ptr, n_minibatch=n, d_grad_logits=self.gl.ptr,
                             d_grad_values=self.gv.ptr, d_partials=self.lp.ptr, d_stats=self.stats.ptr)
        L, stream = _lib.load(), torch.cuda.current_stream(self.dev).cuda_stream
        for rc in (lambda: L.oc_policy_forward(ctypes.byref(pol), ctypes.byref(rows), self.logits.ptr, self.values.ptr, stream),
                   lambda: L.oc_ppo_loss(ctypes.byref(q), stream),
                   lambda: L.oc_policy_backward(ctypes.byref(pol), ctypes.byref(rows), self.gl.ptr, self.gv.ptr, ctypes.byref(grads), self.pp.ptr, stream),
                   lambda: L.oc_adam_step(ctypes.byref(pol), ctypes.byref(grads), ctypes.byref(ad), stream)):
            assert rc() == 0, L.oc_last_error().decode()
        torch.cuda.synchronize(self.dev)

    def results(self):
        return tuple(self.opt.state()) + (self.stats.host(), self.info.host(), LC.flat([f.host() for f in self.opt.g]))

    def intact(self):
        fenced = [self.feats, self.index, self.logits, self.values, self.gl, self.gv, self.lp, self.pp, self.stats, self.info] + [f for f in self.batch if f]
        return self.opt.intact() and all(f.intact() for f in fenced)


def assert_results(x, y, what):
    for name, p, q in zip(("parameters", "first moments", "second moments", "clock", "stats", "info", "gradients"), x, y):
        assert same(p, q), "%s: the %s differ" % (what, name)


@pytest.mark.parametrize("tail,seat,partner_only", (("96_64_64-1rows-indexed-dense", None, False), ("96_64_64-33rows-indexed-dense", "mixed", False),
                                                    ("96_64_64-488rows-indexed-dense", None, False), ("96_64_64-488rows-indexed-dense", "mixed", False),
                                                    ("96_64_64-488rows-indexed-dense", "all0", True), ("136_64_64-257rows-indexed-dense", "mixed", False),
                                                    ("96_64_64-%drows-indexed-zero_tiles" % PC.BIG, "mixed", False)))
def test_g5_one_minibatch_equals_the_four_calls_bit_for_bit(tail, seat, partner_only, gpu):
    c = next(c for c in PC.CASES if c.id.endswith(tail))
    one, four = Update(c, gpu, seat, partner_only=partner_only), Update(c, gpu, seat, partner_only=partner_only)
    one.update()
    four.four_calls()
    what = "%s seat %s" % (c.id, seat)
    assert_results(one.results(), four.results(), what)
    assert one.intact() and four.intact(), what + ": guard bytes written"
    stats, info = one.stats.host()[0], one.info.host()[0]
    idx, b = one.index_host.astype(np.int64), one.batch_host
    inside = (idx >= 0) & (idx < b.S)
    at = np.where(inside, idx, 0)
    learner = inside & (b.actions[at] <= 5) & ((b.seat[at >> 1] != (at & 1)) if b.seat is not None else True)
    assert stats[0] == learner.sum() and not (one.logits.host() == LC.FILL).any() and not (stats == LC.FILL).any() and not (info == LC.FILL).any()
    if c.M >= 8 and not partner_only:
        assert (~inside).sum() >= 2 and len(np.unique(idx[inside])) < inside.sum()  # out-of-range entries and repeats
    if partner_only:  # count 0: the step is skipped, the weights stay
        assert stats[0] == 0 and not stats.any() and info[3] == 1.0 and info[2] == 0.0 and one.opt.clock.host().tolist() == [0.0, 1.0, 1.0, 1.0]
        assert same(one.opt.state().params, LC.flat(PC.arrays_of(c).weights))
    else:
        assert stats[0] > 0 and stats[7] == 1.0 / stats[0] and info[3] == 0.0 and info[2] == float(np.float32(stats[7])) and info[0] > 0
        assert one.opt.clock.host()[0] == 1.0 and not same(one.opt.state().params, LC.flat(PC.arrays_of(c).weights))


def test_g6_an_epoch_equals_its_minibatches_one_by_one_and_repeats(gpu):
    c = next(c for c in PC.CASES if c.id.endswith("96_64_64-488rows-indexed-dense"))
    for seat in (None, "mixed"):
        whole, again, single = (Update(c, gpu, seat, K=3) for _ in range(3))
        M, n = whole.M, len(whole.index_host)
        assert whole.n_stats == 3 and 0 < n - 2 * M < M  # a shorter last minibatch
        whole.update()
        again.update()
        for k in range(3):
            single.update(lo=k * M, n=min(M, n - k * M), M=M, k0=k)  # (K = 1 each, from the weights the one before left)
        assert_results(whole.results(), again.results(), "epoch twice, seat %s" % seat)
        assert_results(whole.results(), single.results(), "epoch against its minibatches, seat %s" % seat)
        assert whole.intact() and single.intact()
        stats, info = whole.stats.host(), whole.info.host()
        assert (stats[:, 0] > 0).all() and not info[:, 3].any() and whole.opt.clock.host()[0] == 3.0 and len({float(x) for x in info[:, 0]}) == 3


# ------------------------------------------------------------------------------------------ G7: one update against the float64 chain
def _chain_f64(weights, feats, index, lossc, b, logits=None, values=None):
    """The float64 chain of one minibatch: (the rows' features, valid, forward [M, 7], loss_f64 on it — or on the given logits and
    values —)"""
    idx = index.astype(np.int64)
    valid = (idx >= 0) & (idx < len(feats))
    xs = np.where(valid[:, None], feats[np.where(valid, idx, 0)], np.float32(0)).astype(np.float32)
    _, _, out = PC.forward_f64(xs, weights)
    out = np.where(valid[:, None], out, 0.0)
    a = types.SimpleNamespace(**vars(b), M=len(idx), logits=out[:, :6] if logits is None else logits, values=out[:, 6] if values is None else values,
                              index=None, first=0, sample=idx)
    return xs, valid, out, PL.loss_f64(lossc, a)


def test_g7_one_update_against_the_float64_chain(gpu):
    from overcooked_ai_amd.learner import PPOLearner
    from overcooked_ai_amd.policy import ActorCritic
    from overcooked_ai_amd.ppo_loss import LearnerBatch

    c = next(c for c in PC.CASES if c.id.endswith("96_64_64-488rows-indexed-dense"))
    a = PC.arrays_of(c)
    S = len(a.features)
    assert S % 2 == 0
    index = np.where(a.unstable, -1, a.index).astype(np.int32)  # the rows on the ReLU edge are silenced: they name no row
    assert a.unstable.sum() <= PC.UNSTABLE_CAP * c.M
    b = _batch_arrays(S, 77, "mixed")
    lr, eps = 1e-2, 1e-2
    lossc = PL.Case("update", c.M, "indexed", 0, "mixed", False, False, False, *LOSS, False, 0)
    policy = ActorCritic.from_weights(*a.weights, device=gpu)
    learner = PPOLearner(policy, lr, clip_param=LOSS[0], vf_clip_param=LOSS[1], vf_loss_coeff=LOSS[2], entropy_coeff=LOSS[3], eps=eps)
    dev = lambda x: torch.from_numpy(x.copy()).to(gpu)  # noqa: E731
    batch = LearnerBatch(dev(b.actions), dev(b.logp_old), dev(b.advantages), dev(b.targets), dev(b.seat), None, None)
    stats, info = learner.update(dev(a.features), batch, dev(index))
    assert stats.shape == (1, 8) and info.shape == (1, 4) and stats.device.type == "cuda"
    stats, info = stats.cpu().numpy()[0], info.cpu().numpy()[0]
    s = learner.scratch(c.M)
    host = lambda t: t.detach().cpu().numpy()  # noqa: E731
    # ---- link 1: the logits and values within policy_cases' bound of the float64 forward pass
    xs, valid, out64, _ = _chain_f64(a.weights, a.features, index, lossc, b)
    got = np.concatenate([host(s["logits"]), host(s["values"])[:, None]], 1)
    assert (np.abs(got - out64) <= PC.forward_bound(xs, a.weights))[valid].all() and not bits(got[~valid]).any()
    # ---- link 2: the loss's raw gradients and stats against loss_f64 on those logits and values
    _, _, _, ref = _chain_f64(a.weights, a.features, index, lossc, b, host(s["logits"]), host(s["values"]))
    near_ratio, near_vf = PL.bands(lossc, ref)
    assert near_ratio.sum() <= max(1, PL.BAND_CAP * c.M) and near_vf.sum() <= max(1, PL.BAND_CAP * c.M)
    assert PL.rel_error(host(s["grad_logits"]), ref.grad_logits, ~near_ratio) <= PL.DEVICE_TOL
    assert PL.rel_error(host(s["grad_values"]), ref.grad_values, ~near_vf) <= PL.DEVICE_TOL
    count = ref.sums[0]
    assert count == stats[0] > 100 and stats[7] == 1.0 / count and PL.rel_error(stats[1:7], ref.stats[1:7]) <= PL.DEVICE_TOL
    # ---- link 3: the raw parameter gradients against backward_f64 on those upstream gradients
    up = np.concatenate([host(s["grad_logits"]), host(s["grad_values"])[:, None]], 1)
    up = np.where(valid[:, None], up, np.float32(0)).astype(np.float32)
    back = PC._backward(xs, a.weights, up, np.float64)
    errs = PC.scaled_errors([host(g) for g in s["grads"]], back)
    assert max(errs) <= PC.DEVICE_FACTOR * PC.F32_ERROR, dict(zip(PC.NAMES, errs))
    # ---- link 4: the parameter change against the float64 Adam on those float64 gradients, within update_bound
    g64 = LC.flat(back.grads) / count
    p_old = LC.flat(a.weights).astype(np.float64)
    st, info64 = LC.adam_f64(LC.state0(a.weights, np.float64), LC.split(LC.flat(back.grads), c.in_dim, c.h1, c.h2), LC.Hyper(lr, 0.9, 0.999, eps, None), 1.0 / count)
    p_new = LC.flat([host(p) for p in policy._params()]).astype(np.float64)
    bound = LC.update_bound(g64, LC.flat(back.scales) / count + 2.0 ** -24 * np.abs(g64), float(np.float32(lr)), float(np.float32(eps)), p_old)
    err = np.abs((p_new - p_old) - (st.params - p_old))
    print("largest |device step - float64 step| / bound %.3g; largest step %.3g, smallest bound %.3g" % ((err / bound).max(), np.abs(st.params - p_old).max(), bound.min()))
    assert (err <= bound).all() and np.abs(st.params - p_old).max() > 100 * bound.min()
    assert info[3] == 0.0 and info[1] == 1.0 and abs(info[0] - info64[0]) <= 1e-3 * info64[0]


# ------------------------------------------------------------------------------------------ G8: a collected buffer end to end
def _f64_updates(weights, feats, index, lossc, b, hyper, n):
    """The value loss before each of n float64 updates on one minibatch (the weights rounded to float32 between them, as they are stored)"""
    dims = (feats.shape[1], weights[0].shape[1], weights[2].shape[1])
    st, out = LC.state0(weights, np.float64), []
    for _ in range(n):
        w = [x.astype(np.float32) for x in LC.split(st.params, *dims)]
        xs, valid, _, ref = _chain_f64(w, feats, index, lossc, b)
        up = np.where(valid[:, None], np.concatenate([ref.grad_logits, ref.grad_values[:, None]], 1), 0.0)
        back = PC._backward(xs, w, up, np.float64)
        out.append(ref.stats[3])
        st, _ = LC.adam_f64(st, LC.split(LC.flat(back.grads), *dims), hyper, ref.stats[7])
    return out


def test_g8_a_collected_buffer_end_to_end(gpu):
    from overcooked_ai_amd.learner import PPOLearner
    from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent
    from overcooked_ai_amd.policy import ActorCritic
    from overcooked_ai_amd.ppo_loss import ppo_loss
    from overcooked_ai_amd.trajectory_buffer import TrajectoryBuffer

    n, T, F = 33, 5, 96
    env = VecOvercookedMultiAgent("cramped_room", n, horizon=4, obs="features", device=gpu, seed=31, reward_shaping_factor=1.0, use_phi=True)
    env.reset()
    policy = ActorCritic(F, seed=11).to(gpu)
    with torch.no_grad():
        for bias in (policy.b1, policy.b2, policy.bp, policy.bv):
            bias.uniform_(-0.5, 0.5, generator=torch.Generator(device=gpu).manual_seed(2))
    buf = TrajectoryBuffer(env, T, keep_obs=True)
    for t in range(T):
        logits, values = policy.act(env.observations("features"))
        env.step_sampled(logits, into=buf.row(t, values))
    buf.last_values.copy_(policy.act(env.observations("features"))[1])
    adv, tgt, mom = buf.advantages(0.99, 0.98)
    batch = buf.learner_batch(adv, tgt, mom)
    S = T * n * 2
    hyper = dict(clip_param=0.05, vf_clip_param=10.0, vf_loss_coeff=0.5, entropy_coeff=0.01)
    perm = buf.permutation(generator=torch.Generator(device=gpu).manual_seed(9))
    assert perm.dtype == torch.int32 and sorted(perm.tolist()) == list(range(S))
    M = S // 3 + 7
    start = [p.detach().clone() for p in policy._params()]
    learner = PPOLearner(policy, 1e-3, max_grad_norm=0.1, **hyper)
    stats, info = learner.epoch(buf.features, batch, perm, M)
    assert stats.shape == (3, 8) and info.shape == (3, 4) and not bool(info[:, 3].any()) and float(learner.adam.clock[0]) == 3.0
    assert float(stats[:, 0].sum()) == S and bool((info[:, 1] <= 1).all())
    # ---- the same pass minibatch by minibatch on a twin: its stats are ppo_loss's on the weights held at that point
    twin = ActorCritic.from_weights(*[p.cpu().numpy() for p in start], device=gpu)
    twin_learner = PPOLearner(twin, 1e-3, max_grad_norm=0.1, **hyper)
    for k in range(3):
        index = perm[k * M:(k + 1) * M]
        with torch.no_grad():
            _, held = ppo_loss(*twin(buf.features, index), batch, index, **hyper)
        s1, i1 = twin_learner.update(buf.features, batch, index)
        assert torch.equal(held.tensor, stats[k]) and torch.equal(s1[0], stats[k]) and torch.equal(i1[0], info[k]), k
    assert all(torch.equal(p, q) for p, q in zip(policy._params(), twin._params()))
    assert not any(torch.equal(p, q) for p, q in zip(policy._params(), start))
    # ---- the value loss of a fixed minibatch falls over 10 updates: first in float64 on the CPU, then on the device
    host = lambda t: t.detach().cpu().numpy()  # noqa: E731
    fixed = perm[:M].contiguous()
    b = types.SimpleNamespace(S=S, actions=host(batch.actions), logp_old=host(batch.logp_old), advantages=host(batch.advantages), targets=host(batch.targets),
                              seat=None, logits_old=None, moments=host(mom))
    lossc = PL.Case("buffer", M, "indexed", 0, "none", True, False, False, 0.05, 10.0, 0.5, 0.01, 0.0, False, 0)
    w0 = [host(p) for p in policy._params()]
    vf64 = _f64_updates(w0, host(buf.features).reshape(S, F), host(fixed), lossc, b, LC.Hyper(1e-3, 0.9, 0.999, 1e-8, 0.1), 11)
    assert vf64[10] < vf64[0], vf64
    vf = [float(learner.update(buf.features, batch, fixed)[0][0, 3]) for _ in range(11)]
    print("value loss of the fixed minibatch: %.6f -> %.6f on the device, %.6f -> %.6f in float64" % (vf[0], vf[10], vf64[0], vf64[10]))
    assert vf[10] < vf[0] and abs(vf[0] - vf64[0]) <= 1e-4 * max(1.0, vf64[0])
