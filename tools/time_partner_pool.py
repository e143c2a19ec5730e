"""Time the partner pool: oc_partner_pool_logits beside what a user had before it.
   python tools/time_partner_pool.py [--out profiles/partner_pool.txt] [n_envs ...]
cramped_room, obs "features" (num_pots = 2: 96 inputs), 96 -> 64 -> 64 -> 6 networks with Glorot weights, drawn start states;
16 384 and 65 536 envs; pools of K = 1, 4 and 16 members; bc_factor 0, 0.5 and 1 (seats and members are drawn once, by the first
call, and kept: the timed calls pass an all-zero done mask).  REPEATS samples of CALLS calls each after a warm-up, by device events
around the calls, the ways of a shape alternating; median (min..max); "host" is the enqueue time of the same calls — where the two
are equal the figure is the host's, not the device's.
  (q) pool.partner_logits(logits)     oc_partner_pool_logits: k_pool_seat, k_sample_scan, k_pool_write, k_pool_logits
  (k) single-policy partner_logits    oc_partner_logits with ONE policy on the same seed: the same seated rows, the same MFMA work
  (t) torch pool                      K masked passes: member mask -> gather of the seated player's row -> F.linear / relu x 3 ->
                                      scatter into the logits (clamp + where: no host synchronisation)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent  # noqa: E402
from overcooked_ai_amd.partner import DensePolicy, PartnerPool  # noqa: E402

REPEATS = 5
CALLS = 100
WARMUP = 20
args = sys.argv[1:]
out_path = os.path.join("profiles", "partner_pool.txt")
if args and args[0] == "--out":
    out_path, args = args[1], args[2:]
sizes = [int(a) for a in args] or [16384, 65536]
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def glorot(rng, fan_in, fan_out):
    lim = np.sqrt(6.0 / (fan_in + fan_out))
    return rng.uniform(-lim, lim, (fan_in, fan_out)).astype(np.float32), rng.uniform(-0.5, 0.5, (fan_out,)).astype(np.float32)


def torch_pool(seat, member, feats, logits, ws, rows):
    p = seat.clamp(max=1).long()
    x = feats[rows, p]
    for m, w in enumerate(ws):
        h = F.relu(F.linear(x, w[0], w[1]))
        h = F.relu(F.linear(h, w[2], w[3]))
        out = F.linear(h, w[4], w[5])
        logits[rows, p] = torch.where((member == m)[:, None], out, logits[rows, p])


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


rng = np.random.default_rng(0)
policies = [DensePolicy(*(glorot(rng, 96, 64) + glorot(rng, 64, 64) + glorot(rng, 64, 6)), device=dev) for _ in range(16)]
tws = [[t.t().contiguous() if t.dim() == 2 else t for t in p.tensors()] for p in policies]  # F.linear takes [out, in]
say("tools/time_partner_pool.py on one device: us per call, cramped_room, obs=features, 96 -> 64 -> 64 -> 6, %d samples of %d calls after %d warm-up calls; median (min..max; host)."
    % (REPEATS, CALLS, WARMUP))
over = []
for n in sizes:
    kw = dict(horizon=400, device=dev, use_phi=False, random_start_pos=True, rnd_obj_prob_thresh=0.35, seed=0, obs="features")
    logits = (torch.randn((8, n, 2, 6), device=dev) * 3.0).contiguous()
    rows = torch.arange(n, device=dev)
    for K in (1, 4, 16):
        for factor in (0.0, 0.5, 1.0):
            pooled = VecOvercookedMultiAgent("cramped_room", n, bc_policy=PartnerPool(policies[:K]), **kw)
            single = VecOvercookedMultiAgent("cramped_room", n, bc_policy=policies[0], **kw)
            for env in (pooled, single):
                env.set_bc_factor(factor)
                env.partner_logits(logits[0])  # seats (and members) drawn here, kept from now on: done stays all zero
            assert torch.equal(pooled.seat, single.seat)
            seated = int((pooled.seat != 255).sum())
            feats = pooled._feat_buffer()
            ways = {"(q) pool partner_logits    ": lambda i: pooled.partner_logits(logits[i % 8]),
                    "(k) single-policy call     ": lambda i: single.partner_logits(logits[i % 8]),
                    "(t) torch, K masked passes ": lambda i: torch_pool(pooled.seat, pooled.member, feats, logits[i % 8], tws[:K], rows)}
            for fn in ways.values():
                for i in range(WARMUP):
                    fn(i)
            times = {k: [] for k in ways}
            for _ in range(REPEATS):
                for k, fn in ways.items():
                    times[k].append(sample(fn))
            say("n=%d K=%d bc_factor=%g: %d seated rows   [%s]" % (n, K, factor, seated, pooled.plan_partner()))
            med, host = {}, {}
            for k in ways:
                t, h = sorted(x[0] for x in times[k]), sorted(x[1] for x in times[k])
                med[k], host[k] = t[len(t) // 2], h[len(h) // 2]
                say("  %s %8.2f us (min %.2f, max %.2f; host %.2f)" % (k, med[k], t[0], t[-1], host[k]))
            q, k1, t = (med[x] for x in ways)
            say("    -> (q) = %.2fx (k), (q) - (k) = %+.2f us; (t) = %.2fx (q)" % (q / k1, q - k1, t / q))
            if q > 2 * k1:
                over.append("n=%d K=%d bc_factor=%g" % (n, K, factor))
            del pooled, single
say("shapes where the pool costs more than twice the single-policy call: %s" % (", ".join(over) if over else "none"))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
