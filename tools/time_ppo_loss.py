"""Time the PPO loss head: oc_ppo_loss (k_ppo_loss + k_ppo_loss_stats) and a torch restatement of the same loss, forward plus backward
to the gradients of the logits and the values, on the same tensors.
   python tools/time_ppo_loss.py [--out profiles/ppo_loss.txt] [--kernel-only] [--envs N] [M ...]
A batch of S = N x 400 x 2 samples (N = 65 536): random actions (1 % the sampler's 255 with a NaN logp), N(0, 2) old logits, seats at
bc_factor 0.5, oc_gae-style moments; minibatches of M = 2^17, 2^20, 2^22 rows whose logits are a 0.05 perturbation of the old ones,
contiguous (from sample 1 000 000) and indexed by the first M entries of a random permutation of the batch; with and without
seat + moments, with and without the old logits (kl_coeff 0.2 with them).  clip 0.05, vf_clip 10, vf_loss_coeff 0.5, entropy_coeff 0.1.
REPEATS samples of CALLS calls each after a warm-up, by device events around the calls, the ways of a shape alternating; median
(min..max); "host" is the enqueue time of the same calls.
  (k) oc_ppo_loss          the C call on preallocated outputs (gradients, partials, stats): what ppo_loss()'s forward launches
  (g) ... gradients only   the same call without d_partials and d_stats: k_ppo_loss without its reduction, and no k_ppo_loss_stats
  (p) ppo_loss + backward  the Python surface: forward (allocating its outputs) and loss.backward() to the logits' and values' .grad
  (t) torch restatement    log_softmax, gather, exp, clamp, min, where, masked mean; torch.autograd.grad to logits and values
Bytes per sample of (k): 24 logits + 4 value + 1 action + 4 logp_old + 4 advantage + 4 target read, 24 + 4 written = 69; + 0.5 (seat),
+ 4 (index), + 24 (old logits); rate = bytes / time against 8 TB/s, for what the kernel asks for — an indexed gather moves a whole
cache line for each of its 1- to 24-byte pieces."""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from overcooked_ai_amd import _lib  # noqa: E402
from overcooked_ai_amd.ppo_loss import LearnerBatch, partial_samples, plan_ppo_loss, ppo_loss  # noqa: E402

REPEATS = 7
HBM_TBS = 8.0
HYPER = dict(clip_param=0.05, vf_clip_param=10.0, vf_loss_coeff=0.5, entropy_coeff=0.1)
args = sys.argv[1:]
out_path, kernel_only, n_envs = os.path.join("profiles", "ppo_loss.txt"), False, 65536
while args and args[0].startswith("--"):
    if args[0] == "--out":
        out_path, args = args[1], args[2:]
    elif args[0] == "--envs":
        n_envs, args = int(args[1]), args[2:]
    elif args[0] == "--kernel-only":
        kernel_only, args = True, args[1:]
    else:
        raise SystemExit("unknown option %s" % args[0])
sizes = [int(a) for a in args] or [2 ** 17, 2 ** 20, 2 ** 22]
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def sample(fn, calls):
    """(us per call by device events, us per call of host enqueue time) over `calls` calls"""
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


def torch_loss(logits, values, batch, index, first, kl_coeff):
    """The same loss in torch float32: (loss, d loss / d logits, d loss / d values)."""
    logits = logits.detach().requires_grad_(True)
    values = values.detach().requires_grad_(True)
    M = logits.shape[0]
    s = index.long() if index is not None else torch.arange(first, first + M, device=logits.device)
    take = (lambda t: t[s]) if index is not None else (lambda t: t[first:first + M])
    act = take(batch.actions).long()
    keep = act <= 5
    if batch.seat is not None:
        keep = keep & (batch.seat[s >> 1].long() != (s & 1))
    A = take(batch.advantages)
    if batch.moments is not None:
        n, m1, m2 = batch.moments
        mean = m1 / n
        std = torch.clamp(torch.sqrt(torch.clamp(m2 / n - mean * mean, min=0.0)), min=1e-4)
        A = ((A.double() - mean) / std).float()
    lp = torch.log_softmax(logits, -1)
    logp = lp.gather(1, act.clamp(max=5)[:, None])[:, 0]
    lpo = torch.where(keep, take(batch.logp_old), 0.0)
    ratio = torch.exp(logp - lpo)
    surr = torch.min(ratio * A, torch.clamp(ratio, 1 - HYPER["clip_param"], 1 + HYPER["clip_param"]) * A)
    H = -(lp.exp() * lp).sum(-1)
    vfc = torch.clamp((values - take(batch.targets)) ** 2, max=HYPER["vf_clip_param"])
    per = -surr + HYPER["vf_loss_coeff"] * vfc - HYPER["entropy_coeff"] * H
    if batch.logits_old is not None:
        lq = torch.log_softmax(take(batch.logits_old), -1)
        per = per + kl_coeff * (lq.exp() * (lq - lp)).sum(-1)
    loss = torch.where(keep, per, 0.0).sum() / keep.sum()
    g_logits, g_values = torch.autograd.grad(loss, (logits, values))
    return loss, g_logits, g_values


S = n_envs * 400 * 2
say("tools/time_ppo_loss.py on one device: us per call, S = %d samples (%d envs x 400 steps x 2), %d samples per way; median (min..max; host)."
    % (S, n_envs, REPEATS))
gen = torch.Generator(device=dev)
gen.manual_seed(0)
actions = torch.randint(0, 6, (S,), device=dev, generator=gen).to(torch.uint8)
invalid = torch.rand((S,), device=dev, generator=gen) < 0.01
actions[invalid] = 255
old = (torch.randn((S, 6), device=dev, generator=gen) * 2).contiguous()
logp_old = torch.log_softmax(old, -1).gather(1, actions.long().clamp(max=5)[:, None])[:, 0].contiguous()
logp_old[invalid] = float("nan")
adv = 0.3 + 1.5 * torch.randn((S,), device=dev, generator=gen)
targets = 3 * torch.randn((S,), device=dev, generator=gen)
draw = torch.randint(0, 4, (S // 2,), device=dev, generator=gen)
seat = torch.where(draw < 2, draw, 255).to(torch.uint8)
players = torch.arange(S, device=dev) & 1
learner = seat.repeat_interleave(2) != players
x = adv.double()[learner]
moments = torch.stack([learner.sum().double(), x.sum(), (x * x).sum()])
perm = torch.randperm(S, device=dev, generator=gen, dtype=torch.int32)
del draw, players, learner, x, invalid
FIRST = 1000000
P = partial_samples()
L = _lib.load()
stream = torch.cuda.current_stream(dev).cuda_stream

for M in sizes:
    grad_logits, grad_values = torch.empty((M, 6), device=dev), torch.empty((M,), device=dev)
    partials, stats = torch.empty(((M + P - 1) // P, 6), device=dev, dtype=torch.float64), torch.empty((8,), device=dev, dtype=torch.float64)
    for mode in ("contiguous", "indexed"):
        index = perm[:M].contiguous() if mode == "indexed" else None
        s = index.long() if index is not None else torch.arange(FIRST, FIRST + M, device=dev)
        logits = (old[s] + 0.05 * torch.randn((M, 6), device=dev, generator=gen)).contiguous()
        values = (targets[s] + 2 * torch.randn((M,), device=dev, generator=gen)).contiguous()
        del s
        for extras in (False, True):
            for with_old in (False, True):
                batch = LearnerBatch(actions, logp_old, adv, targets, seat if extras else None, old if with_old else None,
                                     moments if extras else None)
                kl = 0.2 if with_old else 0.0
                ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
                q = _lib.OcPpoLoss(ptr(actions), ptr(logp_old), ptr(adv), ptr(targets), ptr(batch.seat), ptr(batch.logits_old), ptr(batch.moments),
                                   S, ptr(logits), ptr(values), ptr(index), FIRST if index is None else 0, M, ptr(grad_logits), ptr(grad_values),
                                   ptr(partials), ptr(stats), None, HYPER["clip_param"], HYPER["vf_clip_param"], HYPER["vf_loss_coeff"],
                                   HYPER["entropy_coeff"], kl)

                def kernel(i):
                    if L.oc_ppo_loss(ctypes.byref(q), stream) != 0:
                        raise RuntimeError(L.oc_last_error().decode())

                q_grads = _lib.OcPpoLoss.from_buffer_copy(q)
                q_grads.d_partials = q_grads.d_stats = None

                def grads_only(i):
                    if L.oc_ppo_loss(ctypes.byref(q_grads), stream) != 0:
                        raise RuntimeError(L.oc_last_error().decode())

                lg, vl = logits.clone().requires_grad_(True), values.clone().requires_grad_(True)

                def python(i):
                    lg.grad = vl.grad = None
                    loss, _ = ppo_loss(lg, vl, batch, index, FIRST, kl_coeff=kl, **HYPER)
                    loss.backward()

                def restated(i):
                    torch_loss(logits, values, batch, index, FIRST, kl)

                nbytes = M * (69 + (0.5 if extras else 0) + (4 if index is not None else 0) + (24 if with_old else 0))
                say("M=%d %s%s%s   [%s]" % (M, mode, ", seat + moments" if extras else "", ", old logits" if with_old else "",
                                            plan_ppo_loss(M, index is not None, extras, extras, with_old, False)))
                ways = {"(k) oc_ppo_loss         ": kernel, "(g) ... gradients only  ": grads_only}
                calls = [20, 20]
                if not kernel_only:
                    # the two agree: the mean loss, and the gradients as backward scales them
                    kernel(0)
                    t_loss, t_gl, t_gv = torch_loss(logits, values, batch, index, FIRST, kl)
                    scale = stats[7]
                    # (a ratio within a rounding of a clip edge, or a vf of vf_clip_param, puts a row on either branch: such rows
                    # differ by a whole gradient and are counted, not compared)
                    d_l = (grad_logits.double() * scale - t_gl.double()).abs().max(1).values / t_gl.double().abs().max()
                    d_v = (grad_values.double() * scale - t_gv.double()).abs() / t_gv.double().abs().max()
                    say("  loss %.7f (count %d, clip_frac %.3f), torch %.7f; largest gradient difference / largest gradient: logits %.2g, values %.2g; "
                        "rows on the other branch: %d + %d"
                        % (float(stats[1]), int(stats[0]), float(stats[6]), float(t_loss), float(d_l[d_l < 1e-3].max()), float(d_v[d_v < 1e-3].max()),
                           int((d_l >= 1e-3).sum()), int((d_v >= 1e-3).sum())))
                    ways.update({"(p) ppo_loss + backward ": python, "(t) torch restatement   ": restated})
                    calls += [10, 4]
                med = timed(ways, calls)
                for k, (m, lo, hi, host) in med.items():
                    tail = ""
                    if k.startswith("(k)"):
                        rate = nbytes / m * 1e-6  # TB/s
                        tail = "   %.1f B/sample, %.2f TB/s = %.2f of %.0f TB/s" % (nbytes / M, rate, rate / HBM_TBS, HBM_TBS)
                    say("  %s %10.1f us (min %.1f, max %.1f; host %.1f)%s" % (k, m, lo, hi, host, tail))
                if not kernel_only:
                    ks = list(med)
                    say("    -> (t) / (k) = %.1fx; (t) / (p) = %.1fx" % (med[ks[3]][0] / med[ks[0]][0], med[ks[3]][0] / med[ks[2]][0]))
                del lg, vl
        del logits, values, index
    del grad_logits, grad_values, partials, stats
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
