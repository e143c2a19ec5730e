"""Time the learner's sample index: oc_sample_select and oc_sample_permute beside what a user has without them, and one PPO epoch
fed by either index.
   python tools/time_sample_index.py [--out profiles/sample_index.txt] [n_samples ...]
S = 2^17, 2^22 and 52 428 800 samples (65 536 envs x 400 steps x 2), without seats and fully seated (a partner in every env, the
player drawn per (step, env): L = S / 2); actions valid.  REPEATS samples of CALLS calls each (400 / 200 / 10 of the library's,
40 / 20 / 3 of torch's: every timed window is 3 ms or longer) after a warm-up, by device events around the calls, the ways of a
shape alternating; median (min..max); "host" is the enqueue time of the same calls.
  (s)  select                              k_sample_count + k_sample_scan + k_sample_write
  (p)  permute(samples, L)                 k_sample_permute<IDS=true>: the learner's samples, shuffled
  (pi) permute(None, S)                    k_sample_permute<IDS=false>: a plain permutation of 0 .. S - 1
  (r)  torch.randperm(S)                   what TrajectoryBuffer.permutation() returns today
  (rm) torch.randperm + mask               the learner's samples shuffled, in torch: perm[keep[perm]] (a gather and a boolean-mask
                                           compaction behind the sort)
Floors printed beside them, bytes over 8 TB/s: select reads 1.5 S bytes (1 S without seats) and writes 4 S; permute writes 4 n and
gathers n ids of 4 bytes, each from a line of its own once the ids no longer fit a cache — a floor of bytes, not of lines.
The results are checked before they are timed — ids against torch.nonzero, the index as a permutation of the ids — and a wrong
one ends the run.
Epoch: S = 2^22 samples fully seated, a synthetic batch and 96 random features per sample, PPOLearner.epoch with minibatch 2^17:
  (eo) today's index    permutation(): 32 minibatches, about half of each counted
  (en) the new index    learner_permutation(): 16 minibatches, all of each counted"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from overcooked_ai_amd import sample_index  # noqa: E402
from overcooked_ai_amd.learner import PPOLearner  # noqa: E402
from overcooked_ai_amd.policy import ActorCritic  # noqa: E402
from overcooked_ai_amd.ppo_loss import LearnerBatch  # noqa: E402

REPEATS = 5
HBM_TBS = 8.0
SEED = 0x9E3779B97F4A7C15
args = sys.argv[1:]
out_path = os.path.join("profiles", "sample_index.txt")
if args and args[0] == "--out":
    out_path, args = args[1], args[2:]
sizes = [int(a) for a in args] or [2 ** 17, 2 ** 22, 52428800]
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


say("tools/time_sample_index.py on one device: us per call, %d samples per way; median (min..max; host); floors at %.0f TB/s." % (REPEATS, HBM_TBS))
gen = torch.Generator(device=dev)
gen.manual_seed(0)
for S in sizes:
    actions = torch.randint(0, 6, (S,), device=dev, generator=gen, dtype=torch.uint8)
    for seated in (False, True):
        seat = torch.randint(0, 2, (S // 2,), device=dev, generator=gen, dtype=torch.uint8) if seated else None
        samples = sample_index.select(seat, actions, S)
        L = samples.n
        keep = torch.ones(S, dtype=torch.bool, device=dev)
        if seated:
            keep = seat.repeat_interleave(2) != (torch.arange(S, device=dev) & 1).to(torch.uint8)
        want = torch.nonzero(keep).view(-1).to(torch.int32)
        ok_ids = L == int(want.shape[0]) and bool(torch.equal(samples.ids[:L], want)) and bool((samples.ids[L:] == -1).all())
        index = sample_index.permute(samples, L, SEED, 3)
        ok_perm = bool(torch.equal(torch.sort(index).values, want)) and not bool(torch.equal(index, want))
        del want
        if not (ok_ids and ok_perm):  # wrong results are not timed
            raise SystemExit("S=%d %s: ids equal torch.nonzero: %s; index a permutation of them: %s — nothing timed" % (S, "seated" if seated else "no seats", ok_ids, ok_perm))
        say("S=%d %s: L=%d   [%s]   ids equal torch.nonzero: %s; index a permutation of them: %s"
            % (S, "seated" if seated else "no seats", L, sample_index.plan(S, seat=seated, actions=True, n_out=L, n_learner=L), ok_ids, ok_perm))
        out_l = torch.empty((L,), dtype=torch.int32, device=dev)
        out_s = torch.empty((S,), dtype=torch.int32, device=dev)
        ways = {"(s)  select                 ": lambda i: sample_index.select(seat, actions, S),
                "(p)  permute(samples, L)    ": lambda i: sample_index.permute(samples, L, SEED, i, out=out_l),
                "(pi) permute(None, S)       ": lambda i: sample_index.permute(None, S, SEED, i, out=out_s),
                "(r)  torch.randperm(S)      ": lambda i: torch.randperm(S, dtype=torch.int32, device=dev),
                "(rm) torch.randperm + mask  ": lambda i: (lambda p: p[keep[p.long()]])(torch.randperm(S, dtype=torch.int32, device=dev))}
        calls = (400, 400, 400, 40, 40) if S <= 2 ** 17 else (200, 200, 200, 20, 20) if S <= 2 ** 22 else (10, 10, 10, 3, 3)  # windows of 3 ms and more
        med = timed(ways, calls)
        floors = {"(s) ": (1.5 if seated else 1.0) * S + 4 * S, "(p) ": 8 * L, "(pi)": 4 * S}
        for k, (m, lo, hi, host) in med.items():
            nbytes = floors.get(k[:4])
            floor = "   floor %.1f us (%d bytes): %.2f of it" % (nbytes / HBM_TBS * 1e-6, nbytes, nbytes / HBM_TBS * 1e-6 / m) if nbytes else ""
            say("  %s %10.1f us (min %.1f, max %.1f; host %.1f)%s" % (k, m, lo, hi, host, floor))
        ks = list(med)
        say("    -> (r) / (pi) = %.1fx; (rm) / ((s) + (p)) = %.1fx; (rm) / (p) = %.1fx"
            % (med[ks[3]][0] / med[ks[2]][0], med[ks[4]][0] / (med[ks[0]][0] + med[ks[1]][0]), med[ks[4]][0] / med[ks[1]][0]))
        del samples, index, keep, out_l, out_s, seat
        torch.cuda.empty_cache()
    del actions

S, F, M = 2 ** 22, 96, 2 ** 17
say("epoch: S=%d fully seated, %d features, minibatch %d, PPOLearner.epoch; 3 epochs per sample" % (S, F, M))
actions = torch.randint(0, 6, (S,), device=dev, generator=gen, dtype=torch.uint8)
seat = torch.randint(0, 2, (S // 2,), device=dev, generator=gen, dtype=torch.uint8)
features = torch.randn((S, F), device=dev, generator=gen)
f32 = lambda: torch.randn((S,), device=dev, generator=gen)  # noqa: E731
adv = f32()
moments = torch.stack([torch.tensor(float(S // 2), device=dev, dtype=torch.float64), adv.double().sum() / 2, (adv.double() ** 2).sum() / 2])
batch = LearnerBatch(actions, -1.8 + 0.1 * f32(), adv, f32(), seat, None, moments)
policy = ActorCritic(F, seed=1).to(dev)
learner = PPOLearner(policy, 5e-5, clip_param=0.05, vf_clip_param=10.0, vf_loss_coeff=1e-4, entropy_coeff=0.1, max_grad_norm=0.1)
samples = sample_index.select(seat, actions, S)
L = samples.n
old = torch.randperm(S, dtype=torch.int32, device=dev)
new = sample_index.permute(samples, L, SEED, 0)
counted = lambda stats: "%d minibatches, %.0f..%.0f samples counted in each, %.0f in all" % (  # noqa: E731
    stats.shape[0], float(stats[:, 0].min()), float(stats[:, 0].max()), float(stats[:, 0].sum()))
say("  today's index: %s" % counted(learner.epoch(features, batch, old, M)[0]))
say("  the new index: %s" % counted(learner.epoch(features, batch, new, M)[0]))
if not bool(torch.equal(torch.sort(new).values, torch.nonzero(seat.repeat_interleave(2) != (torch.arange(S, device=dev) & 1).to(torch.uint8)).view(-1).to(torch.int32))):
    raise SystemExit("epoch: the new index is no permutation of the learner's samples — nothing timed")
ways = {"(eo) epoch, permutation()         ": lambda i: learner.epoch(features, batch, old, M),
        "(en) epoch, learner_permutation() ": lambda i: learner.epoch(features, batch, new, M)}
med = timed(ways, (3, 3))
for k, (m, lo, hi, host) in med.items():
    say("  %s %10.1f us (min %.1f, max %.1f; host %.1f)" % (k, m, lo, hi, host))
ks = list(med)
say("    -> (eo) / (en) = %.2fx for the same %d learner samples" % (med[ks[0]][0] / med[ks[1]][0], L))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
