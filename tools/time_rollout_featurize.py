"""Time K transitions + featurize_state of every step (oc_rollout_featurize): the single kernel against the same entry point
on its step-by-step path (oc_rollout_random(1) + oc_featurize per step: kernels as they were before k_rollout_featurize, the baseline):
   python tools/time_rollout_featurize.py [layout] [n_envs] [K] [num_pots]
Both paths run in one process, alternating, REPEATS samples of CALLS calls each after a warm-up, timed with device events.  (a) sets `one_kernel`;
(b) clears it and lifts the planner's fill threshold out of reach with the tuning knob OC_ROLLOUT_FEATURIZE_FILL, which only a
library built with -DOC_AMD_TUNING reads: unless OC_AMD_LIB names one, overcooked_ai_amd/rollout_featurize_tune.so is built first
(python tools/build_variants.py rollout_featurize_tune=-DOC_AMD_TUNING builds it ahead of time).
Per path: us per step (median, min..max over the repeats), n_envs * (2 * total * 4 + 17) * K bytes over that time as TB/s and as a
share of 8 TB/s; then the plan the planner picks by default for this shape, and the rate of oc_output_stores_only writing the same
number of bytes as rewards and flags."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if not os.environ.get("OC_AMD_LIB"):
    from overcooked_ai_amd import build

    tune = os.path.join(build.PKG, "rollout_featurize_tune.so")
    if not os.path.exists(tune) or any(os.path.getmtime(p) > os.path.getmtime(tune) for p in build._source_files()):
        build.build_extension(force=True, defines=("-DOC_AMD_TUNING",), out=tune)
    os.environ["OC_AMD_LIB"] = tune

import torch  # noqa: E402

from overcooked_ai_amd.vec_env import VecOvercookedEnv  # noqa: E402

REPEATS = 7
CALLS = 10  # calls of K steps per timed sample
KNOB = "OC_ROLLOUT_FEATURIZE_FILL"
layout = sys.argv[1] if len(sys.argv) > 1 else "cramped_room"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
K = int(sys.argv[3]) if len(sys.argv) > 3 else 40
num_pots = int(sys.argv[4]) if len(sys.argv) > 4 else 2
dev = torch.device("cuda:0")
env = VecOvercookedEnv(layout, n, horizon=400, device=dev, auto_reset=True, seed=0)
total = 2 * (num_pots * 10 + 26) + 4
feats = torch.empty((K, n, 2, total), dtype=torch.float32, device=dev)
rew = torch.zeros((K, n, 4), dtype=torch.float32, device=dev)
fl = torch.zeros((K, n), dtype=torch.uint8, device=dev)
step_bytes = n * (2 * total * 4 + 17)


def select(one_kernel):
    env.one_kernel = one_kernel
    if one_kernel:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = str(2**31 - 1)


def run(one_kernel):
    """us per step over CALLS calls of K steps"""
    select(one_kernel)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        env.rollout_featurize(K, feats, rew, fl, num_pots=num_pots)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (CALLS * K) * 1e3


plans = {}
for one in (True, False):
    select(one)
    plans[one] = env.plan_rollout_featurize(K, num_pots)
assert plans[True].startswith("k_rollout_featurize<") and plans[False].startswith("step by step: "), plans
for _ in range(2):
    run(True), run(False)
times = {True: [], False: []}
for _ in range(REPEATS):
    for one in (True, False):
        times[one].append(run(one))
print("%s n=%d K=%d num_pots=%d (%d floats per row, %.1f MB per step)" % (layout, n, K, num_pots, total, step_bytes / 1e6))
med = {}
for one, name in ((True, "(a) one kernel  "), (False, "(b) step by step")):
    t = sorted(times[one])
    med[one] = t[len(t) // 2]
    rate = step_bytes / med[one] / 1e6
    print("%s %7.2f us per step (min %.2f, max %.2f over %d repeats) -> %.2f TB/s = %.0f %% of 8 TB/s   [%s]"
          % (name, med[one], t[0], t[-1], REPEATS, rate, rate / 8 * 100, plans[one]))
spread = max(max(times[o]) - min(times[o]) for o in (True, False))
env.one_kernel = False
os.environ.pop(KNOB, None)
default = env.plan_rollout_featurize(K, num_pots)
faster = med[True] < med[False]
print("default plan: %s -> the %s path; the faster one is %s by %.2f us per step (spread of the repeats: %.2f us)"
      % (default[:default.index(">") + 1], "one-kernel" if default.startswith("k_rollout_featurize<") else "step-by-step",
         "(a)" if faster else "(b)", abs(med[True] - med[False]), spread))
# the same bytes as nothing but reward and flag stores (17 bytes per env-step), 8 steps per launch
ns, ks = (step_bytes + 16) // 17, 8
r2 = torch.empty((ks, ns, 4), dtype=torch.float32, device=dev)
f2 = torch.empty((ks, ns), dtype=torch.uint8, device=dev)
for timed in (False, True):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        assert env.lib.oc_output_stores_only(ns, ks, r2.data_ptr(), f2.data_ptr(), 0, None) == 0
    e1.record()
    torch.cuda.synchronize()
us = e0.elapsed_time(e1) / (5 * ks) * 1e3
print("oc_output_stores_only, %d bytes per step: %.2f us per step -> %.2f TB/s" % (ns * 17, us, ns * 17 / us / 1e6))
