"""Time behaviour cloning on the device: oc_bc_loss (k_bc_loss + k_bc_loss_stats) alone, and `BCLearner.update` / `.epoch`
(oc_bc_update), each beside the path a user has without them, in the same run.
   python tools/time_bc.py [--out profiles/bc.txt] [--loss-only] [--learner-only]
96 -> 64 -> 64 -> 6 + 1, Glorot weights; a pool of 2^22 feature rows drawn like featurize_state's entries with an action byte each
(skewed towards STAY, as human data is); lr 1e-3, max_grad_norm 0.1, six class weights.
  loss       M = 2^17, 2^20, 2^22 rows, contiguous and indexed (a random permutation)
             (k) oc_bc_loss               the C call on preallocated outputs: gradients, partials, stats
             (b) ... gradients only       the same call without d_partials and d_stats: k_bc_loss without its reduction
             (e) ... evaluation           no gradient arrays: sums and stats only
             (q) oc_ppo_loss, grads only  k_ppo_loss's gradient pass on the same rows: the kernel k_bc_loss is shaped after
             (t) torch                    F.cross_entropy(logits, labels, weight) + backward to the logits' .grad
             bytes per row: the least the pass must move — (b) 24 + 1 read, 24 + 4 written; (q) 24 + 4 + 1 + 4 + 4 + 4 read, 24 + 4
             written; an indexed pass reads 4 more
  minibatch  M = 64 (the reference's batch size), 4 096, 2^17, 2^20 indexed rows
             (u) BCLearner.update         one C call: forward, cross-entropy, backward, clipped Adam
             (t) torch                    ActorCritic + F.cross_entropy + backward + clip_grad_norm_ + torch.optim.Adam
  epoch      16 minibatches of each of those sizes
             (E) BCLearner.epoch          one C call for the sixteen
             (t) torch, sixteen times
REPEATS samples of CALLS calls each after a warm-up, by device events around the calls, the ways of a shape alternating; median
(min..max); "host" is the host's time over the same calls (the enqueue time; where it is the device time the way is enqueue-bound)."""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from overcooked_ai_amd import _lib  # noqa: E402
from overcooked_ai_amd.bc import BCLearner, partial_samples, plan_bc_loss, plan_bc_update  # noqa: E402
from overcooked_ai_amd.policy import ActorCritic  # noqa: E402

REPEATS = 7
IN, H1, H2 = 96, 64, 64
LR, CLIP = 1e-3, 0.1
args = sys.argv[1:]
out_path, do_loss, do_learner = os.path.join("profiles", "bc.txt"), True, True
while args and args[0].startswith("--"):
    if args[0] == "--out":
        out_path, args = args[1], args[2:]
    elif args[0] == "--loss-only":
        do_learner, args = False, args[1:]
    elif args[0] == "--learner-only":
        do_loss, args = False, args[1:]
    else:
        raise SystemExit("unknown option %s" % args[0])
if not torch.cuda.is_available():
    raise SystemExit("tools/time_bc.py needs a GPU: a timing taken anywhere else says nothing")
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def sample(fn, calls):
    """(us per call by device events, us per call of host time) over `calls` calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    h0 = time.perf_counter()
    for i in range(calls):
        fn(i)
    h1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3, (h1 - h0) / calls * 1e6


def timed(ways, calls):
    for fn, c in zip(ways.values(), calls):
        for i in range(min(c, 3)):
            fn(i)
    times = {k: [] for k in ways}
    for _ in range(REPEATS):
        for (k, fn), c in zip(ways.items(), calls):
            times[k].append(sample(fn, c))
    med = {}
    for k in ways:
        t, h = sorted(x[0] for x in times[k]), sorted(x[1] for x in times[k])
        med[k] = (t[len(t) // 2], t[0], t[-1], h[len(h) // 2])
    return med


def report(med, bytes_per_call=None):
    for k, (m, lo, hi, host) in med.items():
        rate = "" if not bytes_per_call or k not in bytes_per_call else "; %.0f GB/s of the least bytes" % (bytes_per_call[k] / m * 1e-3)
        say("  %s %10.1f us (min %.1f, max %.1f; host %.1f%s)" % (k, m, lo, hi, host, rate))


gen = torch.Generator(device=dev)
gen.manual_seed(0)
S = 2 ** 22
SKEW = torch.tensor((0.05, 0.05, 0.08, 0.08, 0.64, 0.10), device=dev)
actions = torch.multinomial(SKEW, S, replacement=True, generator=gen).to(torch.uint8)
labels = actions.long()
weights = (1.0 / (6.0 * SKEW)).float().contiguous()
perm = torch.randperm(S, device=dev, generator=gen, dtype=torch.int32)
L = _lib.load()
stream = torch.cuda.current_stream(dev).cuda_stream
say("tools/time_bc.py on one device: us per call, %d samples per way; median (min..max; host)." % REPEATS)

# ------------------------------------------------------------------------------------------ the loss head alone
if do_loss:
    logits_all = (2 * torch.randn((S, 6), device=dev, generator=gen)).contiguous()
    values = torch.randn((S,), device=dev, generator=gen)
    logp_old = torch.log_softmax(logits_all + 0.05 * torch.randn((S, 6), device=dev, generator=gen), -1).gather(1, labels[:, None])[:, 0].contiguous()
    adv, targets = torch.randn((S,), device=dev, generator=gen), torch.randn((S,), device=dev, generator=gen)
    P = partial_samples()
    gl, gv = torch.empty((S, 6), device=dev), torch.empty((S,), device=dev)
    partials, stats = torch.empty(((S + P - 1) // P, 6), dtype=torch.float64, device=dev), torch.empty((8,), dtype=torch.float64, device=dev)
    for M in (2 ** 17, 2 ** 20, 2 ** 22):
        for indexed in (False, True):
            index = perm[:M].contiguous() if indexed else None
            ip = index.data_ptr() if indexed else None
            logits = logits_all[:M]
            bc = lambda g, p: _lib.OcBcLoss(actions.data_ptr(), weights.data_ptr(), S, logits.data_ptr(), ip, 0, M, gl.data_ptr() if g else None,  # noqa: E731
                                            gv.data_ptr() if g else None, None, partials.data_ptr() if p else None, stats.data_ptr() if p else None)
            q_full, q_grads, q_eval = bc(True, True), bc(True, False), bc(False, True)
            q_ppo = _lib.OcPpoLoss(actions.data_ptr(), logp_old.data_ptr(), adv.data_ptr(), targets.data_ptr(), None, None, None, S, logits.data_ptr(),
                                   values.data_ptr(), ip, 0, M, gl.data_ptr(), gv.data_ptr(), None, None, None, 0.05, 10.0, 0.5, 0.1, 0.0)

            def c_call(fn, q):
                def go(i):
                    if fn(ctypes.byref(q), stream) != 0:
                        raise RuntimeError(L.oc_last_error().decode())
                return go

            lab = labels[index.long()] if indexed else labels[:M]
            leaf = logits.clone().requires_grad_(True)

            def torch_way(i):
                leaf.grad = None
                F.cross_entropy(leaf, lab, weight=weights, reduction="sum").div(M).backward()

            KK, B, E, Q, T = "(k) oc_bc_loss            ", "(b) ... gradients only    ", "(e) ... evaluation        ", "(q) oc_ppo_loss, grads only", "(t) torch                 "
            say("loss head, %d %s rows   [%s]" % (M, "indexed" if indexed else "contiguous", plan_bc_loss(M, indexed, True)))
            calls = 20 if M <= 2 ** 20 else 10
            med = timed({KK: c_call(L.oc_bc_loss, q_full), B: c_call(L.oc_bc_loss, q_grads), E: c_call(L.oc_bc_loss, q_eval),
                         Q: c_call(L.oc_ppo_loss, q_ppo), T: torch_way}, [calls] * 5)
            extra = 4 if indexed else 0
            report(med, {B: M * (53 + extra), Q: M * (69 + extra), KK: M * (53 + extra), E: M * (25 + extra)})
            say("    -> (t) / (k) = %.1fx by device time; (q) / (b) = %.2fx (bytes %.2fx)" % (med[T][0] / med[KK][0], med[Q][0] / med[B][0], (69 + extra) / (53 + extra)))
    del logits_all, values, logp_old, adv, targets, gl, gv, partials

# ------------------------------------------------------------------------------------------ the learner
if do_learner:
    pool = torch.randint(-6, 7, (S, IN), device=dev, generator=gen).float()
    pool[torch.rand((S, IN), device=dev, generator=gen) < 0.4] = 0

    def new_policy():
        policy = ActorCritic(IN, H1, H2, seed=1).to(dev)
        with torch.no_grad():
            for b in (policy.b1, policy.b2, policy.bp, policy.bv):
                b.uniform_(-0.5, 0.5, generator=torch.Generator(device=dev).manual_seed(5))
        return policy

    ours_policy, torch_policy = new_policy(), new_policy()
    learner = BCLearner(ours_policy, LR, class_weights=weights.cpu(), max_grad_norm=CLIP)
    torch_opt = torch.optim.Adam(torch_policy.parameters(), LR)

    def torch_minibatch(index):
        torch_opt.zero_grad()
        logits, _ = torch_policy(pool, index)
        F.cross_entropy(logits, labels[index.long()], weight=weights, reduction="sum").div(index.shape[0]).backward()
        torch.nn.utils.clip_grad_norm_(torch_policy.parameters(), CLIP)
        torch_opt.step()

    U, E, T = "(u) BCLearner.update      ", "(E) BCLearner.epoch       ", "(t) torch                 "
    K = 16
    for M in (64, 4096, 2 ** 17, 2 ** 20):
        index = perm[:M].contiguous()
        say("one minibatch of %d indexed rows   [%s]" % (M, plan_bc_update(M, M, IN, H1, H2, True)))
        calls = 20 if M <= 4096 else 10 if M <= 2 ** 17 else 4
        med = timed({U: lambda i: learner.update(pool, actions, index), T: lambda i: torch_minibatch(index)}, [calls, calls])
        report(med)
        say("    -> (t) / (u) = %.1fx by device time, %.1fx by host time" % (med[T][0] / med[U][0], med[T][3] / med[U][3]))
        whole = torch.randint(0, S, (K * M,), device=dev, generator=gen, dtype=torch.int32)  # (16 x 2^20 entries: rows repeat)
        cuts = [whole[k * M:(k + 1) * M] for k in range(K)]

        def torch_epoch(i):
            for cut in cuts:
                torch_minibatch(cut)

        say("an epoch of %d x %d indexed rows (us per epoch)" % (K, M))
        calls = 5 if M <= 4096 else 3 if M <= 2 ** 17 else 1
        med = timed({E: lambda i: learner.epoch(pool, actions, whole, M), T: torch_epoch}, [calls, calls])
        report(med)
        say("    -> (t) / (E) = %.1fx by device time, %.1fx by host time; per minibatch %.1f us against %.1f us" % (
            med[T][0] / med[E][0], med[T][3] / med[E][3], med[E][0] / K, med[T][0] / K))
    stats, info = learner.epoch(pool, actions, whole, M)
    held = learner.evaluate(pool, actions, perm[:4096].contiguous())
    say("    the last epoch's last minibatch: count %d, loss %.4f, accuracy %.4f, gradient norm %.4f, skipped %d of %d; evaluate on 4096 rows: loss %.4f, accuracy %.4f"
        % (int(stats[-1, 0]), float(stats[-1, 1]), float(stats[-1, 2]), float(info[-1, 0]), int(info[:, 3].sum()), K, float(held.loss), float(held.accuracy)))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
