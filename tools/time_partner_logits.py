"""Time the behaviour-cloning partner of the training env: k_partner_logits alone, step_sampled with and without a partner, and the
torch equivalent of the partner.
   python tools/time_partner_logits.py [--out profiles/partner_logits.txt] [n_envs ...]
cramped_room, obs "both" (u8 image and featurize_state, num_pots = 2: 96 inputs), the reference's 96 -> 64 -> 64 -> 6 network with
Glorot weights, use_phi on, drawn start states, horizon 400; 65 536, 32 768 and 16 384 envs; bc_factor 0, 0.5 and 1 (the seats are
drawn once, by the first call, and kept: the timed calls pass an all-zero done mask).  REPEATS samples of CALLS calls each after a
warm-up, by device events around the calls, the ways of a shape alternating; median (min..max); "host" is the enqueue time of the same
calls — where the two are equal the figure is the host's, not the device's.
  (k) partner_logits(logits)          oc_partner_logits alone: one launch, k_partner_logits
  (e) a one-element torch fill        the nearest thing to an empty launch: what any launch costs in this loop
  (p) step_sampled, with the partner  partner_logits, then oc_multi_agent_step_sample
  (s) step_sampled, without           an env built without a policy, same commit
  (t) torch partner                   seat mask -> gather of the seated player's row -> F.linear / relu x 3 -> scatter into the logits
                                      (clamp + where: no host synchronisation), and the sum of its kernels' device times from
                                      torch.profiler in a pass of its own
Derived per shape: the FLOP rate of (k) — seated rows x 2 x (96 * 64 + 64 * 64 + 64 * 32), the padded network the kernel computes —
against the 157.3 TF f32 matrix peak of the MI355X; (p) - (s) against (k); (t) against (k)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent  # noqa: E402
from overcooked_ai_amd.partner import DensePolicy  # noqa: E402

REPEATS = 7
CALLS = 200
WARMUP = 30
PEAK_TF = 157.3
args = sys.argv[1:]
out_path = os.path.join("profiles", "partner_logits.txt")
if args and args[0] == "--out":
    out_path, args = args[1], args[2:]
sizes = [int(a) for a in args] or [65536, 32768, 16384]
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def glorot(rng, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, (fan_in, fan_out)).astype(np.float32), rng.uniform(-0.5, 0.5, (fan_out,)).astype(np.float32)


def torch_partner(seat, feats, logits, w, rows):
    p = seat.clamp(max=1).long()
    x = feats[rows, p]
    h = F.relu(F.linear(x, w[0], w[1]))
    h = F.relu(F.linear(h, w[2], w[3]))
    out = F.linear(h, w[4], w[5])
    logits[rows, p] = torch.where((seat != 255)[:, None], out, logits[rows, p])


def sample(fn):
    """(us per call by device events, us per call of host enqueue time) over CALLS calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    h0 = time.perf_counter()
    for i in range(CALLS):
        fn(i)
    h1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3, (h1 - h0) / CALLS * 1e6


def kernel_time_sum(fn):
    """us per call: the device times of every kernel of CALLS calls, summed (torch.profiler, a pass of its own); None if unavailable"""
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for i in range(CALLS):
                fn(i)
            torch.cuda.synchronize()
        total = sum(ev.self_device_time_total for ev in prof.key_averages() if ev.device_type == torch.autograd.DeviceType.CUDA)  # kernels only
        return total / CALLS if total > 0 else None
    except Exception as e:  # noqa: BLE001
        say("    (torch.profiler not usable here: %s)" % e)
        return None


rng = np.random.default_rng(0)
weights = glorot(rng, 96, 64) + glorot(rng, 64, 64) + glorot(rng, 64, 6)
policy = DensePolicy(*weights, device=dev)
tw = [t.t().contiguous() if t.dim() == 2 else t for t in policy.tensors()]  # F.linear takes [out, in]
say("tools/time_partner_logits.py on one device: us per call, cramped_room, obs=both (u8), 96 -> 64 -> 64 -> 6, %d samples of %d calls after %d warm-up calls; median (min..max; host)."
    % (REPEATS, CALLS, WARMUP))
losses = []
for n in sizes:
    kw = dict(horizon=400, reward_shaping_factor=1.0, device=dev, use_phi=True, random_start_pos=True, rnd_obj_prob_thresh=0.35, seed=0,
              obs="both", obs_dtype=torch.uint8)
    plain = VecOvercookedMultiAgent("cramped_room", n, **kw)
    logits = (torch.randn((8, n, 2, 6), device=dev) * 3.0).contiguous()
    rows = torch.arange(n, device=dev)
    one = torch.zeros((1,), device=dev)
    for factor in (0.0, 0.5, 1.0):
        env = VecOvercookedMultiAgent("cramped_room", n, bc_policy=policy, **kw)
        env.set_bc_factor(factor)
        env.partner_logits(logits[0])  # seats drawn here, kept from now on (done is all zero between the timed calls)
        seated = int((env.seat != 255).sum())
        alone = VecOvercookedMultiAgent("cramped_room", n, bc_policy=policy, **kw)  # (k) and (t) on an env that does not step
        alone.set_bc_factor(factor)
        alone.partner_logits(logits[0])
        feats = alone._feat_buffer()
        ways = {"(k) partner_logits alone   ": lambda i: alone.partner_logits(logits[i % 8]),
                "(e) one-element torch fill ": lambda i: one.fill_(1.0),
                "(p) step_sampled, partner  ": lambda i: env.step_sampled(logits[i % 8]),
                "(s) step_sampled, without  ": lambda i: plain.step_sampled(logits[i % 8]),
                "(t) torch partner          ": lambda i: torch_partner(alone.seat, feats, logits[i % 8], tw, rows)}
        for fn in ways.values():
            for i in range(WARMUP):
                fn(i)
        times = {k: [] for k in ways}
        for _ in range(REPEATS):
            for k, fn in ways.items():
                times[k].append(sample(fn))
        say("n=%d bc_factor=%g: %d seated rows   [%s; %s]" % (n, factor, seated, env.plan_partner(), env.plan_sampled()))
        med = {}
        for k in ways:
            t, h = sorted(x[0] for x in times[k]), sorted(x[1] for x in times[k])
            med[k] = t[len(t) // 2]
            say("  %s %8.2f us (min %.2f, max %.2f; host %.2f)" % (k, med[k], t[0], t[-1], h[len(h) // 2]))
        k, e, p, s, t = (med[x] for x in ways)
        ksum = kernel_time_sum(ways["(t) torch partner          "])
        flop = seated * 2.0 * (96 * 64 + 64 * 64 + 64 * 32)
        say("    -> (k): %.2f TFLOP/s = %.1f %% of the %.1f TF f32 matrix peak; (k) - (e) = %+.2f us; (p) - (s) = %+.2f us; (t) wall %.2f us = %.2fx (k), its kernels alone %s"
            % (flop / k * 1e-6, 100 * flop / k * 1e-6 / PEAK_TF, PEAK_TF, k - e, p - s, t, t / k, "%.2f us = %.2fx (k)" % (ksum, ksum / k) if ksum else "not measured"))
        if k > t:
            losses.append("n=%d bc_factor=%g" % (n, factor))
        del env, alone
    del plain
say("shapes where k_partner_logits is slower than the torch partner (wall): %s" % (", ".join(losses) if losses else "none"))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
