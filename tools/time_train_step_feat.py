"""Time one step of the batched training environment WITH the featurize_state observation (VecOvercookedMultiAgent.step):
   python tools/time_train_step_feat.py [--out profiles/train_step_feat.txt] [layout ...]
Three ways to the same data, as three envs in one process, alternating, REPEATS samples of CALLS calls each after a warm-up, timed
with device events around the calls (the host's enqueue time of the same calls is shown beside it: where the two are equal the
figure is the host's, not the device's):
  (a) obs="features", one_kernel=True    oc_multi_agent_step_featurize forced onto k_train_step_feat
  (b) obs="features"                     the same entry point on the plan it picks by default
  (c) obs="bc"                           the way before that entry point: step() = oc_multi_agent_step (k_train_step1) followed by
                                         observations("bc") (k_featurize of the state just written)
for each layout (default: cramped_room and asymmetric_advantages) at 16 384, 32 768 and 65 536 envs, num_pots = 2, use_phi on, drawn
start states, horizon 400.  Per way: us per call as median (min..max), the plan; per shape: which of (a) and (c) is faster, by how
much, and the larger spread of the two.  The table goes to --out as well."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from overcooked_ai_amd.multi_agent import VecOvercookedMultiAgent  # noqa: E402

REPEATS = 9
CALLS = 300
WARMUP = 40
SIZES = (16384, 32768, 65536)
args = sys.argv[1:]
out_path = os.path.join("profiles", "train_step_feat.txt")
if args and args[0] == "--out":
    out_path, args = args[1], args[2:]
layouts = args or ["cramped_room", "asymmetric_advantages"]
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def sample(env, acts):
    """(us per call by device events, us per call of host enqueue time) over CALLS calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    h0 = time.perf_counter()
    for i in range(CALLS):
        env.step(acts[i % len(acts)])
    h1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3, (h1 - h0) / CALLS * 1e6


say("tools/time_train_step_feat.py on one device: us per VecOvercookedMultiAgent.step call, num_pots = 2, use_phi on, drawn starts, horizon 400;")
say("three envs in one process, alternating, %d samples of %d calls each after %d warm-up calls (device events); median (min..max), host = enqueue time of the same calls." % (REPEATS, CALLS, WARMUP))
say("(a) obs=\"features\" forced onto k_train_step_feat; (b) obs=\"features\" on its default plan; (c) obs=\"bc\": k_train_step1, then k_featurize (the way before).")
for layout in layouts:
    for n in SIZES:
        kw = dict(horizon=400, reward_shaping_factor=1.0, device=dev, use_phi=True, random_start_pos=True, rnd_obj_prob_thresh=0.35, seed=0)
        envs = {"(a) one kernel ": VecOvercookedMultiAgent(layout, n, obs="features", one_kernel=True, **kw),
                "(b) default    ": VecOvercookedMultiAgent(layout, n, obs="features", **kw),
                "(c) two before ": VecOvercookedMultiAgent(layout, n, obs="bc", **kw)}
        acts = torch.randint(0, 6, (16, n, 2), dtype=torch.uint8, device=dev)
        plans = {k: e.plan() for k, e in envs.items()}
        assert plans["(a) one kernel "].startswith("k_train_step_feat<") and "k_featurize" not in plans["(c) two before "], plans
        plans["(c) two before "] += " + " + envs["(c) two before "].venv.featurize_plan(2)
        for e in envs.values():
            for i in range(WARMUP):
                e.step(acts[i % len(acts)])
        times = {k: [] for k in envs}
        for _ in range(REPEATS):
            for k, e in envs.items():
                times[k].append(sample(e, acts))
        say("%s n=%d (%.1f MB of features per call)" % (layout, n, n * 2 * 96 * 4 / 1e6))
        med, spread = {}, {}
        for k in envs:
            t = sorted(x[0] for x in times[k])
            h = sorted(x[1] for x in times[k])
            med[k], spread[k] = t[len(t) // 2], t[-1] - t[0]
            say("%s %7.2f us per call (min %.2f, max %.2f; host %.2f)   [%s]" % (k, med[k], t[0], t[-1], h[len(h) // 2], plans[k]))
        a, c = "(a) one kernel ", "(c) two before "
        say("    -> %s is faster by %.2f us per call; spread of the repeats: %.2f us; the default plan is the %s path"
            % ("(a)" if med[a] < med[c] else "(c)", abs(med[a] - med[c]), max(spread[a], spread[c]),
               "one-kernel" if plans["(b) default    "].startswith("k_train_step_feat<") else "two-launch"))
        del envs
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
