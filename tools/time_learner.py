"""Time the learner's update: `PPOLearner.update` / `.epoch` (oc_ppo_update) and `Adam.step` (oc_adam_step, k_adam_step), each
against the path a user of `ActorCritic` had before them, in the same run.
   python tools/time_learner.py [--out profiles/learner.txt] [M ...]
96 -> 64 -> 64 -> 6 + 1, Glorot weights; a pool of feature rows drawn like featurize_state's entries and a learner batch over it, as
tools/time_policy.py draws them; lr 1e-4, max_grad_norm 0.1 (the reference trainer's grad_clip).
  minibatch  M = 4 096, 2^17, 2^20 indexed rows
             (u) PPOLearner.update                       one C call: forward, loss, backward, clipped Adam
             (p) the parent's path                       ActorCritic + ppo_loss + loss.backward() + clip_grad_norm_ + torch.optim.Adam
  epoch      16 minibatches of 4 096 rows
             (e) PPOLearner.epoch                        one C call for the sixteen
             (p) the parent's path, sixteen times
  optimiser  the eight gradients given
             (k) oc_adam_step, the C call on prepared structs
             (a) learner.Adam.step()
             (t) clip_grad_norm_ + torch.optim.Adam.step()
REPEATS samples of CALLS calls each after a warm-up, by device events around the calls, the ways of a shape alternating; median
(min..max); "host" is the host's time over the same calls (the enqueue time; where it is the device time the way is enqueue-bound)."""
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from overcooked_ai_amd import _lib  # noqa: E402
from overcooked_ai_amd.learner import Adam, PPOLearner, plan_adam, plan_update  # noqa: E402
from overcooked_ai_amd.policy import ActorCritic  # noqa: E402
from overcooked_ai_amd.ppo_loss import LearnerBatch, ppo_loss  # noqa: E402

REPEATS = 7
IN, H1, H2 = 96, 64, 64
LR, CLIP = 1e-4, 0.1
args = sys.argv[1:]
out_path = os.path.join("profiles", "learner.txt")
while args and args[0].startswith("--"):
    if args[0] == "--out":
        out_path, args = args[1], args[2:]
    else:
        raise SystemExit("unknown option %s" % args[0])
sizes = [int(a) for a in args] or [4096, 2 ** 17, 2 ** 20]
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


def report(med):
    for k, (m, lo, hi, host) in med.items():
        say("  %s %10.1f us (min %.1f, max %.1f; host %.1f)" % (k, m, lo, hi, host))


def new_policy():
    policy = ActorCritic(IN, H1, H2, seed=1).to(dev)
    with torch.no_grad():
        for b in (policy.b1, policy.b2, policy.bp, policy.bv):
            b.uniform_(-0.5, 0.5, generator=torch.Generator(device=dev).manual_seed(5))
    return policy


gen = torch.Generator(device=dev)
gen.manual_seed(0)
POOL = max(sizes + [16 * 4096]) + 1000000
pool = torch.randint(-6, 7, (POOL, IN), device=dev, generator=gen).float()
pool[torch.rand((POOL, IN), device=dev, generator=gen) < 0.4] = 0
perm = torch.randperm(POOL, device=dev, generator=gen, dtype=torch.int32)
ours_policy, parent_policy = new_policy(), new_policy()
S = POOL
actions = torch.randint(0, 6, (S,), device=dev, generator=gen).to(torch.uint8)
with torch.no_grad():
    old, old_values = ours_policy(pool)
logp_old = torch.log_softmax(old, -1).gather(1, actions.long()[:, None])[:, 0].contiguous()
adv = 0.3 + 1.5 * torch.randn((S,), device=dev, generator=gen)
targets = (old_values + 2 * torch.randn((S,), device=dev, generator=gen)).contiguous()
del old
batch = LearnerBatch(actions, logp_old, adv, targets, None, None, None)
hyper = dict(clip_param=0.05, vf_clip_param=10.0, vf_loss_coeff=0.5, entropy_coeff=0.1)
learner = PPOLearner(ours_policy, LR, max_grad_norm=CLIP, **hyper)
parent_opt = torch.optim.Adam(parent_policy.parameters(), LR)
say("tools/time_learner.py on one device: us per call, %d -> %d -> %d -> 6 + 1, %d samples per way; median (min..max; host)." % (IN, H1, H2, REPEATS))


def parent_minibatch(index):
    parent_opt.zero_grad()
    loss, _ = ppo_loss(*parent_policy(pool, index), batch, index, **hyper)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(parent_policy.parameters(), CLIP)
    parent_opt.step()


# ------------------------------------------------------------------------------------------ one minibatch
U, P = "(u) PPOLearner.update      ", "(p) the parent's path      "
for M in sizes:
    index = perm[:M].contiguous()
    say("one minibatch of %d indexed rows   [%s]" % (M, plan_update(M, M, IN, H1, H2)))
    med = timed({U: lambda i: learner.update(pool, batch, index), P: lambda i: parent_minibatch(index)}, [10, 10] if M <= 2 ** 17 else [5, 5])
    report(med)
    say("    -> (p) / (u) = %.1fx by device time, %.1fx by host time" % (med[P][0] / med[U][0], med[P][3] / med[U][3]))

# ------------------------------------------------------------------------------------------ an epoch
K, M = 16, 4096
index = perm[:K * M].contiguous()
cuts = [index[k * M:(k + 1) * M] for k in range(K)]


def parent_epoch(i):
    for cut in cuts:
        parent_minibatch(cut)


E = "(e) PPOLearner.epoch       "
say("an epoch of %d x %d indexed rows (us per epoch)" % (K, M))
med = timed({E: lambda i: learner.epoch(pool, batch, index, M), P: parent_epoch}, [5, 5])
report(med)
say("    -> (p) / (e) = %.1fx by device time, %.1fx by host time; per minibatch %.1f us against %.1f us" % (
    med[P][0] / med[E][0], med[P][3] / med[E][3], med[E][0] / K, med[P][0] / K))
stats, info = learner.epoch(pool, batch, index, M)
say("    the epoch's last minibatch: count %d, loss %.4f, gradient norm %.4f, clip factor %.4f, skipped %d of %d" % (
    int(stats[-1, 0]), float(stats[-1, 1]), float(info[-1, 0]), float(info[-1, 1]), int(info[:, 3].sum()), K))

# ------------------------------------------------------------------------------------------ the optimiser alone
a_policy, t_policy = new_policy(), new_policy()
for pol in (a_policy, t_policy):
    for p in pol.parameters():
        p.grad = 0.01 * torch.randn(p.shape, device=dev, generator=gen)
a_opt, t_opt = Adam(a_policy, LR, max_grad_norm=CLIP), torch.optim.Adam(t_policy.parameters(), LR)
a_opt.step()
L = _lib.load()
_, c_pol, c_grads, c_adam = a_opt._call
stream = torch.cuda.current_stream(dev).cuda_stream


def c_call(i):
    if L.oc_adam_step(ctypes.byref(c_pol), ctypes.byref(c_grads), ctypes.byref(c_adam), stream) != 0:
        raise RuntimeError(L.oc_last_error().decode())


def torch_pair(i):
    torch.nn.utils.clip_grad_norm_(t_policy.parameters(), CLIP)
    t_opt.step()


KC, A, T = "(k) oc_adam_step           ", "(a) learner.Adam.step      ", "(t) clip_grad_norm_ + Adam "
say("the optimiser step alone, the gradients given   [%s]" % plan_adam(IN, H1, H2))
med = timed({KC: c_call, A: lambda i: a_opt.step(), T: torch_pair}, [50, 50, 20])
report(med)
say("    -> (t) / (a) = %.1fx by device time, %.1fx by host time; (t) / (k) = %.1fx" % (med[T][0] / med[A][0], med[T][3] / med[A][3], med[T][0] / med[KC][0]))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
