"""Time the fused behaviour-cloning epoch (oc_bc_epoch_fused, `fused=True`) beside the staged path (oc_bc_update, `fused=False`) in
the same run, the two ways alternating.
   python tools/time_bc_fused.py [--out profiles/bc_fused.txt] [--stamps]
96 -> 64 -> 64 -> 6 + 1, Glorot weights; a pool of 2^16 feature rows drawn like featurize_state's entries with an action byte each
(skewed towards STAY); lr 1e-3, max_grad_norm 0.1, six class weights: tools/time_bc.py's learner section at the sizes the fused
kernel serves.
  minibatch  one minibatch of 1, 32, 64, 128 indexed rows: BCLearner.update(..., fused=False) against fused=True
  epoch      16 and 400 minibatches of 64 (the reference's batch size and, at 400, about its pass): BCLearner.epoch
REPEATS samples of CALLS calls each after a warm-up, by device events around the calls; median (min..max); "host" is the host's time
over the same calls.  Both learners start from the same weights and make the same calls: at the end their parameters are compared.
--stamps (a library built with -DOC_AMD_TUNING, named by OC_AMD_LIB): where a fused minibatch's time goes, from the cycle counts
lane 0 leaves at the ends of the kernel's phases; shares of the minibatch, medians over the minibatches of an epoch of 64 x 64 rows."""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from overcooked_ai_amd import _lib  # noqa: E402
from overcooked_ai_amd.bc import BCLearner, plan_bc_epoch_fused  # noqa: E402
from overcooked_ai_amd.policy import ActorCritic  # noqa: E402

REPEATS = 9
IN, H1, H2 = 96, 64, 64
LR, CLIP = 1e-3, 0.1
args = sys.argv[1:]
out_path, stamps = os.path.join("profiles", "bc_fused.txt"), False
while args and args[0].startswith("--"):
    if args[0] == "--out":
        out_path, args = args[1], args[2:]
    elif args[0] == "--stamps":
        stamps, args = True, args[1:]
    else:
        raise SystemExit("unknown option %s" % args[0])
if not torch.cuda.is_available():
    raise SystemExit("tools/time_bc_fused.py needs a GPU: a timing taken anywhere else says nothing")
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
    for _ in range(calls):
        fn()
    h1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3, (h1 - h0) / calls * 1e6


def timed(ways, calls):
    for fn in ways.values():
        for _ in range(3):
            fn()
    times = {k: [] for k in ways}
    for _ in range(REPEATS):
        for k, fn in ways.items():
            times[k].append(sample(fn, calls))
    med = {}
    for k in ways:
        t, h = sorted(x[0] for x in times[k]), sorted(x[1] for x in times[k])
        med[k] = (t[len(t) // 2], t[0], t[-1], h[len(h) // 2])
    return med


gen = torch.Generator(device=dev)
gen.manual_seed(0)
S = 2 ** 16
SKEW = torch.tensor((0.05, 0.05, 0.08, 0.08, 0.64, 0.10), device=dev)
actions = torch.multinomial(SKEW, S, replacement=True, generator=gen).to(torch.uint8)
weights = (1.0 / (6.0 * SKEW)).float().contiguous()
pool = torch.randint(-6, 7, (S, IN), device=dev, generator=gen).float()
pool[torch.rand((S, IN), device=dev, generator=gen) < 0.4] = 0


def new_learner():
    policy = ActorCritic(IN, H1, H2, seed=1).to(dev)
    with torch.no_grad():
        for b in (policy.b1, policy.b2, policy.bp, policy.bv):
            b.uniform_(-0.5, 0.5, generator=torch.Generator(device=dev).manual_seed(5))
    return BCLearner(policy, LR, class_weights=weights.cpu(), max_grad_norm=CLIP)


if stamps:
    L = _lib.load()
    if not hasattr(L, "oc_bc_epoch_fused_stamps"):
        raise SystemExit("--stamps needs a library built with -DOC_AMD_TUNING (python -m overcooked_ai_amd.build is the default build; see build_extension's defines)")
    K, M, NS = 64, 64, 6
    learner = new_learner()
    index = torch.randint(0, S, (K * M,), device=dev, generator=gen, dtype=torch.int32)
    buf = torch.zeros((K, NS), dtype=torch.int64, device=dev)
    L.oc_bc_epoch_fused_stamps.argtypes = [ctypes.c_void_p]
    L.oc_bc_epoch_fused_stamps.restype = None
    learner.epoch(pool, actions, index, M, fused=True)  # (warm-up, no stamps)
    L.oc_bc_epoch_fused_stamps(buf.data_ptr())
    learner.epoch(pool, actions, index, M, fused=True)
    torch.cuda.synchronize()
    L.oc_bc_epoch_fused_stamps(None)
    t = buf.cpu().numpy().astype("float64")
    d = t[:, 1:] - t[:, :-1]
    whole = (t[1:, 0] - t[:-1, 0])
    share = d / d.sum(1, keepdims=True)
    import numpy as np

    names = ("staging", "forward", "head", "backward and wavefront sum", "Adam")
    say("where a fused minibatch's time goes: %d minibatches of %d rows, %d inputs, one launch; lane 0's cycle counter at the ends of the phases" % (K, M, IN))
    for j, name in enumerate(names):
        say("  %-28s %5.1f %% of the minibatch (median; min %.1f, max %.1f), %.0f counts" % (name, 100 * np.median(share[1:, j]), 100 * share[1:, j].min(),
                                                                                         100 * share[1:, j].max(), np.median(d[1:, j])))
    say("  a minibatch, start to start: %.0f counts (median; the first of the launch left out)" % np.median(whole[1:]))
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
    raise SystemExit(0)

staged, fused = new_learner(), new_learner()
say("tools/time_bc_fused.py on one device: us per call, %d samples per way, the ways alternating; median (min..max; host)." % REPEATS)
A, B = "(s) staged, fused=False", "(f) fused=True         "


def verdict(med, per=1):
    s, f = med[A], med[B]
    spread = s[2] - s[1]
    say("  %s %10.1f us (min %.1f, max %.1f; host %.1f)" % (A, s[0], s[1], s[2], s[3]))
    say("  %s %10.1f us (min %.1f, max %.1f; host %.1f)" % (B, f[0], f[1], f[2], f[3]))
    say("    -> staged / fused = %.2fx by device time; per minibatch %.1f us against %.1f us; the staged figure's spread in this run is %.1f us: fused is %s"
        % (s[0] / f[0], s[0] / per, f[0] / per, spread, "faster by more than that" if s[0] - f[0] > spread else "NOT faster by more than that"))


for M in (1, 32, 64, 128):
    index = torch.randint(0, S, (M,), device=dev, generator=gen, dtype=torch.int32)
    say("one minibatch of %d indexed rows   [%s]" % (M, plan_bc_epoch_fused(M, M, IN, H1, H2, True)))
    verdict(timed({A: lambda: staged.update(pool, actions, index), B: lambda: fused.update(pool, actions, index, fused=True)}, 50))
for K, calls in ((16, 10), (400, 2)):
    index = torch.randint(0, S, (K * 64,), device=dev, generator=gen, dtype=torch.int32)
    say("an epoch of %d x 64 indexed rows (us per epoch)   [%s]" % (K, plan_bc_epoch_fused(K * 64, 64, IN, H1, H2, True)))
    verdict(timed({A: lambda: staged.epoch(pool, actions, index, 64), B: lambda: fused.epoch(pool, actions, index, 64, fused=True)}, calls), K)
torch.cuda.synchronize()
equal = all(torch.equal(p, q) for p, q in zip(staged.policy._params(), fused.policy._params())) and torch.equal(staged.adam.clock, fused.adam.clock)
say("after the same calls on both learners: parameters and clock equal bit for bit: %s (steps %d, skipped %d)" % (equal, int(fused.adam.clock[0]), int(fused.adam.clock[3])))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
if not equal:
    raise SystemExit("the two paths differ")
