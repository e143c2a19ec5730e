"""Time the outcome table of a collected batch: oc_outcome_table (k_outcomes + k_outcome_sum) against the torch restatement a user
would write today, in the same run and on the same arrays.
   python tools/time_outcomes.py [--out profiles/outcomes.txt] [--kernel-only] [n_envs ...]
(--kernel-only: without the torch ways, for an A/B of libraries built with -DOC_OUT_B=<steps per prefetch block>, chosen by OC_AMD_LIB)
done at rate 1/400 (a 400-step horizon with staggered phases) or, "equal", every env done on the same step once per 400 steps (T = 50:
on the last step); ep_returns random integers as the env produces them; with seats: per-step seats and members of a pool of 3 at
bc_factor 0.5; 16 384 and 65 536 envs x 50 and 400 steps.  REPEATS samples per way after a warm-up, by device events around CALLS calls,
CALLS chosen per way so that a timed window is at least 3 ms, the ways of a shape alternating; median (min..max); "host" is the enqueue
time of the same calls.
  (o)   outcome_table(done, ep)                          k_outcomes<SEAT=false, MEMBER=false, ENV=false> + k_outcome_sum
  (osm) outcome_table(done, ep, seat, member, 3)         k_outcomes<SEAT=true, MEMBER=true, ENV=false> + k_outcome_sum
  (ose) ... per_env=True                                 k_outcomes<SEAT=true, MEMBER=true, ENV=true> + k_outcome_sum
  (oeq) (osm) on the "equal" done pattern                64 turns per wavefront on the done steps
  (t)   torch restatement, no seats                      a mask, nonzero, a gather of the done rows, an index_add per column, scatter_reduce
                                                         for min and max
  (tsm) torch restatement, seats and members             + the group index of the gathered rows
Both ways allocate their outputs inside the call (the table, the scratch; torch its temporaries).  The torch restatement waits for the
device inside nonzero(): its "host" time is its whole time.
Bytes: per env-step 1 (done) [+ 2 (seat, member)], + 16 per done row; share = the time those bytes take at 8 TB/s over the time measured."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from overcooked_ai_amd.outcomes import outcome_table, plan  # noqa: E402

REPEATS = 7
WINDOW_US = 3000.0
HBM_TBS = 8.0
K = 3
args = sys.argv[1:]
out_path = os.path.join("profiles", "outcomes.txt")
if args and args[0] == "--out":
    out_path, args = args[1], args[2:]
kernel_only = "--kernel-only" in args
args = [a for a in args if a != "--kernel-only"]
sizes = [int(a) for a in args] or [16384, 65536]
horizons = (50, 400)
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def sample(fn, calls):
    """(us per call by device events, us per call of host enqueue time, us of the whole window) over `calls` calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    h0 = time.perf_counter()
    for i in range(calls):
        fn(i)
    h1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    window = e0.elapsed_time(e1) * 1e3
    return window / calls, (h1 - h0) / calls * 1e6, window


def torch_table(done, ep, seat, member, n_members):
    """The table as a user would compute it with torch today: [G + 1, 8] float64."""
    idx = (done.view(-1) != 0).nonzero().squeeze(1)
    rows = ep.view(-1, 4)[idx].double()
    if seat is None:
        G = 1
        g = torch.zeros_like(idx)
    else:
        G = 1 + 2 * n_members
        s, m = seat.view(-1)[idx].long(), member.view(-1)[idx].long()
        g = torch.where(s == 255, 0, torch.where((s <= 1) & (m < n_members), 1 + 2 * m + s, G))
    R = rows[:, 0] + rows[:, 1]
    attributed = g < G
    cols = torch.zeros((8, G + 1), dtype=torch.float64, device=done.device)
    cols[3], cols[4] = float("inf"), float("-inf")
    cols[0].index_add_(0, g, torch.ones_like(R))
    ga, Ra, rows_a = g[attributed], R[attributed], rows[attributed]
    cols[1].index_add_(0, ga, Ra)
    cols[2].index_add_(0, ga, Ra * Ra)
    cols[3].scatter_reduce_(0, ga, Ra, "amin")
    cols[4].scatter_reduce_(0, ga, Ra, "amax")
    cols[5].index_add_(0, ga, rows_a[:, 2])
    cols[6].index_add_(0, ga, rows_a[:, 3])
    cols[7].index_add_(0, ga, rows_a[:, 0])
    return cols.t().contiguous()


def timed(ways):
    calls = {}
    for k, fn in ways.items():
        for i in range(3):
            fn(i)
        calls[k] = 4
        while sample(fn, calls[k])[2] < WINDOW_US * 1.25:  # (a quarter above the 3 ms every timed window must reach)
            calls[k] = calls[k] * 3 // 2 + 1
    times = {k: [] for k in ways}
    for _ in range(REPEATS):
        for k, fn in ways.items():
            times[k].append(sample(fn, calls[k]))
    med = {}
    for k in ways:
        t, h = sorted(x[0] for x in times[k]), sorted(x[1] for x in times[k])
        med[k] = (t[len(t) // 2], t[0], t[-1], h[len(h) // 2], calls[k], min(x[2] for x in times[k]))
    return med


say("tools/time_outcomes.py on one device: us per call, a pool of %d, %d samples per way, every window at least %.0f ms; median (min..max; host)."
    % (K, REPEATS, WINDOW_US / 1000))
gen = torch.Generator(device=dev)
gen.manual_seed(0)
slower = []
for n in sizes:
    for T in horizons:
        phase = torch.randint(0, 400, (n,), device=dev, generator=gen)
        t_idx = torch.arange(T, device=dev)[:, None]
        done = ((t_idx + phase[None, :]) % 400 == 399).to(torch.uint8).contiguous()
        equal = ((t_idx % 400) == min(T, 400) - 1).to(torch.uint8).expand(T, n).contiguous()
        sparse = 20.0 * torch.randint(0, 12, (T, n, 2), device=dev, generator=gen)
        shaped = 3.0 * torch.randint(0, 40, (T, n, 2), device=dev, generator=gen) + 5.0 * torch.randint(0, 40, (T, n, 2), device=dev, generator=gen)
        ep = torch.cat([sparse, shaped], dim=2).float().contiguous()
        draw = torch.randint(0, 4, (T, n), device=dev, generator=gen)
        seat = torch.where(draw < 2, draw, 255).to(torch.uint8)
        member = torch.where(seat == 255, 255, torch.randint(0, K, (T, n), device=dev, generator=gen)).to(torch.uint8)
        del sparse, shaped, draw
        # the two agree: integer data, every sum exact
        got = outcome_table(done, ep, seat, member, K).table
        want = torch_table(done, ep, seat, member, K)
        same = bool(torch.equal(got, want))
        say("n=%d T=%d   [%s]   %d episodes; torch restatement equal: %s" % (n, T, plan(n, T, True, True, K), int(got[:, 0].sum()), same))
        ways = {"(o)   outcome_table                 ": lambda i: outcome_table(done, ep),
                "(osm) outcome_table, seat + member  ": lambda i: outcome_table(done, ep, seat, member, K),
                "(ose) ... and the env table         ": lambda i: outcome_table(done, ep, seat, member, K, per_env=True),
                "(oeq) (osm), equal horizons         ": lambda i: outcome_table(equal, ep, seat, member, K),
                "(t)   torch restatement             ": lambda i: torch_table(done, ep, None, None, 1),
                "(tsm) torch, seat + member          ": lambda i: torch_table(done, ep, seat, member, K)}
        if kernel_only:
            ways = {k: fn for k, fn in ways.items() if k.startswith("(o")}
        med = timed(ways)
        for k, (m, lo, hi, host, calls, window) in med.items():
            which = equal if k.startswith("(oeq)") else done
            nbytes = T * n * (1 if k.startswith(("(o) ", "(t) ")) else 3) + 16 * int((which != 0).sum()) + (32 * n if k.startswith("(ose)") else 0)
            ideal = nbytes / (HBM_TBS * 1e6)  # us
            say("  %s %9.1f us (min %.1f, max %.1f; host %.1f; %d calls, window >= %.1f ms)   %.1f MB: %.1f us at %.0f TB/s = %.2f of the time"
                % (k, m, lo, hi, host, calls, window / 1000, nbytes / 1e6, ideal, HBM_TBS, ideal / m))
        ks = list(med)
        if kernel_only:
            continue
        say("    -> (t) / (o) = %.1fx; (tsm) / (osm) = %.1fx; equal horizons (oeq) - (osm) = %+.1f us; env table (ose) - (osm) = %+.1f us"
            % (med[ks[4]][0] / med[ks[0]][0], med[ks[5]][0] / med[ks[1]][0], med[ks[3]][0] - med[ks[1]][0], med[ks[2]][0] - med[ks[1]][0]))
        for kernel, restatement in ((ks[0], ks[4]), (ks[1], ks[5])):
            if med[kernel][0] > med[restatement][0]:
                slower.append("n=%d T=%d %s" % (n, T, kernel.strip()))
        torch.cuda.empty_cache()
if not kernel_only:
    say("slower than the torch restatement at: %s" % (", ".join(slower) if slower else "no measured shape"))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
