"""Time the advantages of a collected batch: oc_gae (k_gae), a torch restatement of the same f32 recurrence, and the collection loop
that fills the batch.
   python tools/time_gae.py [--out profiles/gae.txt] [n_envs ...]
Random rewards (f64), values (f32), done at rate 1/400 and, with seats, per-episode seats at bc_factor 0.5; gamma 0.99, lambda 0.98;
16 384 and 65 536 envs x 50 and 400 steps.  REPEATS samples of CALLS calls each after a warm-up, by device events around the calls,
the ways of a shape alternating; median (min..max); "host" is the enqueue time of the same calls.
  (g)  gae()                                  oc_gae alone: k_gae<SEAT=false, MOM=false>
  (gs) gae(seat=...)                          k_gae<SEAT=true, MOM=false>
  (gm) gae(seat=..., moments=True)            k_gae<SEAT=true, MOM=true> + k_gae_moments
  (t)  torch restatement                      a reverse loop over T of elementwise f32 ops (where for the select and the seats) into
                                              preallocated outputs
  (tm) torch restatement + masked moments     + count, sum and sum of squares of the learner samples in f64 (what a masked mean / var
                                              computes)
Bytes: per env-step 16 (rewards) + 8 (values) + 1 (done) [+ 1 (seat)] read, 16 written; rate = bytes / time against 8 TB/s.
Collection, per step at the same n_envs (obs "features", cramped_room, no partner; T = 50 rows):
  (ci) step_sampled(logits, into=buf.row(t, values))
  (cc) step_sampled(logits) + the copies a user would write: shaped, done, actions, logp and values into rows of their own buffers"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from overcooked_ai_amd.gae import gae, plan_gae  # noqa: E402
from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent  # noqa: E402
from overcooked_ai_amd.trajectory_buffer import TrajectoryBuffer  # noqa: E402

REPEATS = 5
HBM_TBS = 8.0
args = sys.argv[1:]
out_path = os.path.join("profiles", "gae.txt")
if args and args[0] == "--out":
    out_path, args = args[1], args[2:]
sizes = [int(a) for a in args] or [16384, 65536]
horizons = (50, 400)
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


def torch_gae(rewards, values, done, last, seat, g, gl, adv, tgt, moments):
    T = rewards.shape[0]
    carried = torch.zeros_like(last)
    vn = last
    players = torch.arange(2, device=rewards.device, dtype=torch.uint8)
    for t in range(T - 1, -1, -1):
        r = rewards[t].float()
        v = values[t]
        a_run = ((r + g * vn) - v) + gl * carried
        A = torch.where(done[t][:, None] != 0, r - v, a_run)
        target = A + v
        if seat is not None:
            partner = seat[t][:, None] == players
            A = torch.where(partner, 0.0, A)
            target = torch.where(partner, 0.0, target)
        adv[t] = A
        tgt[t] = target
        carried, vn = A, v
    if moments:
        x = adv.double()
        if seat is not None:
            live = seat[:, :, None] != players
            x = torch.where(live, x, 0.0)
            count = live.sum()
        else:
            count = x.numel()
        return count, x.sum(), (x * x).sum()
    return None


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


say("tools/time_gae.py on one device: us per call, gamma 0.99, lambda 0.98, %d samples per way; median (min..max; host)." % REPEATS)
gen = torch.Generator(device=dev)
gen.manual_seed(0)
for n in sizes:
    for T in horizons:
        rewards = (torch.rand((T, n, 2), device=dev, generator=gen, dtype=torch.float64) - 0.5) * 10
        values = (torch.rand((T, n, 2), device=dev, generator=gen) - 0.5) * 10
        last = (torch.rand((n, 2), device=dev, generator=gen) - 0.5) * 10
        done = (torch.rand((T, n), device=dev, generator=gen) < 1.0 / 400).to(torch.uint8)
        draw = torch.randint(0, 4, (T, n), device=dev, generator=gen)  # 0 / 1: the partner's player (half of the envs), else none
        draw = torch.where(draw < 2, draw, 255).to(torch.uint8)
        episode = torch.cumsum(torch.cat([torch.zeros((1, n), device=dev, dtype=torch.long), done[:-1].long()]), 0)  # episode index per step
        first = torch.zeros((T, n), device=dev, dtype=torch.long)
        first[1:] = torch.where(done[:-1] != 0, torch.arange(1, T, device=dev)[:, None], 0)
        first = torch.cummax(first, 0).values  # the step at which the episode of step t began
        seat = torch.gather(draw, 0, first).contiguous()
        del episode, first, draw
        out = (torch.empty((T, n, 2), device=dev), torch.empty((T, n, 2), device=dev))
        g, gl = 0.99, float(torch.tensor(0.99, dtype=torch.float32) * torch.tensor(0.98, dtype=torch.float32))
        # the two agree (bit for bit where torch rounds each operation once, as the header does)
        a_k, t_k, m_k = gae(rewards, values, done, 0.99, 0.98, last_values=last, seat=seat, moments=True, out=out)
        a_t, t_t = torch.empty_like(a_k), torch.empty_like(t_k)
        m_t = torch_gae(rewards, values, done, last, seat, g, gl, a_t, t_t, True)
        same = bool(torch.equal(a_k.view(torch.int32), a_t.view(torch.int32))) and bool(torch.equal(t_k.view(torch.int32), t_t.view(torch.int32)))
        say("n=%d T=%d   [%s]   torch restatement bit-equal: %s; moments kernel (%.0f, %.6e, %.6e), torch (%.0f, %.6e, %.6e)"
            % (n, T, plan_gae(n, T, seat=True, moments=True), same, *[float(x) for x in m_k], *[float(x) for x in m_t]))
        ways = {"(g)  gae                      ": lambda i: gae(rewards, values, done, 0.99, 0.98, last_values=last, out=out),
                "(gs) gae, seats               ": lambda i: gae(rewards, values, done, 0.99, 0.98, last_values=last, seat=seat, out=out),
                "(gm) gae, seats, moments      ": lambda i: gae(rewards, values, done, 0.99, 0.98, last_values=last, seat=seat, moments=True, out=out),
                "(t)  torch restatement, seats ": lambda i: torch_gae(rewards, values, done, last, seat, g, gl, a_t, t_t, False),
                "(tm) torch, seats, moments    ": lambda i: torch_gae(rewards, values, done, last, seat, g, gl, a_t, t_t, True)}
        med = timed(ways, (10, 10, 10, 2, 2))
        for k, (m, lo, hi, host) in med.items():
            nbytes = T * n * (41 + (0 if k.startswith("(g) ") else 1))
            rate = nbytes / m * 1e-6  # TB/s
            say("  %s %10.1f us (min %.1f, max %.1f; host %.1f)   %.2f TB/s = %.2f of %.0f TB/s" % (k, m, lo, hi, host, rate, rate / HBM_TBS, HBM_TBS))
        ks = list(med)
        say("    -> (t) / (gs) = %.1fx; (tm) / (gm) = %.1fx; moments cost (gm) - (gs) = %+.1f us"
            % (med[ks[3]][0] / med[ks[1]][0], med[ks[4]][0] / med[ks[2]][0], med[ks[2]][0] - med[ks[1]][0]))
        del rewards, values, last, done, seat, out, a_k, t_k, a_t, t_t
        torch.cuda.empty_cache()

say("collection loop, per step: step_sampled(into=row) against step_sampled + five copies; cramped_room, obs=features, T = 50 rows, 4 rounds of 50 steps per sample")
for n in sizes:
    T = 50
    kw = dict(horizon=400, reward_shaping_factor=1.0, device=dev, use_phi=True, seed=0, obs="features")
    env_i, env_c = VecOvercookedMultiAgent("cramped_room", n, **kw), VecOvercookedMultiAgent("cramped_room", n, **kw)
    buf = TrajectoryBuffer(env_i, T)
    mine = TrajectoryBuffer(env_c, T)  # (the user's own buffers: the same tensors, filled by copies)
    logits = (torch.randn((8, n, 2, 6), device=dev) * 3.0).contiguous()
    values = torch.randn((n, 2), device=dev)

    def into(i):
        t = i % T
        env_i.step_sampled(logits[i % 8], into=buf.row(t, values))

    def copies(i):
        t = i % T
        _, shaped, done, infos = env_c.step_sampled(logits[i % 8])
        mine.rewards[t].copy_(shaped)
        mine.done[t].copy_(done)
        mine.actions[t].copy_(infos["actions"])
        mine.logp[t].copy_(infos["logp"])
        mine.values[t].copy_(values)

    med = timed({"(ci) step_sampled(into=row)   ": into, "(cc) step_sampled + 5 copies  ": copies}, (200, 200))
    say("n=%d   [%s]" % (n, env_i.plan_sampled()))
    for k, (m, lo, hi, host) in med.items():
        say("  %s %8.2f us per step (min %.2f, max %.2f; host %.2f)" % (k, m, lo, hi, host))
    ks = list(med)
    say("    -> (cc) - (ci) = %+.2f us per step" % (med[ks[1]][0] - med[ks[0]][0]))
    del env_i, env_c, buf, mine
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
