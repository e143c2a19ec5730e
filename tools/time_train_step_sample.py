"""Time one step of the batched training environment with a policy in the loop: logits in, sampled actions, log-probabilities and the
next observation out.
   python tools/time_train_step_sample.py [--out profiles/train_step_sample.txt] [layout ...]
Three ways to the same data, as three envs in one process, alternating, REPEATS samples of CALLS calls each after a warm-up, timed
with device events around the calls (the host's enqueue time of the same calls is shown beside it: where the two are equal the
figure is the host's, not the device's):
  (a) step_sampled(logits)                        oc_multi_agent_step_sample: the step kernel draws the actions itself (one launch)
  (b) sample_actions(logits), then step(actions)  oc_sample_actions (k_sample_actions), then the step on its own plan
  (c) torch, then step(actions)                   Categorical(logits=logits, validate_args=False).sample(), .log_prob() and a cast
                                                  to uint8 — what a caller did before these entry points (validate_args=False: the
                                                  default's check of the logits waits for the device)
for each layout (default: cramped_room and asymmetric_advantages) at 16 384, 32 768 and 65 536 envs, with obs "ppo" (the u8 lossless
encoding) and obs "features" (featurize_state, num_pots = 2), use_phi on, drawn start states, horizon 400.  Per way: us per call as
median (min..max), the plan; per shape: (a) against (b) with the larger spread of the two — the rule of the planner: fused stays the
default wherever (a) is not slower than (b) by more than that spread — and (a) against (c).  The table goes to --out as well."""
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
out_path = os.path.join("profiles", "train_step_sample.txt")
if args and args[0] == "--out":
    out_path, args = args[1], args[2:]
layouts = args or ["cramped_room", "asymmetric_advantages"]
dev = torch.device("cuda:0")
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def fused(env, logits):
    env.step_sampled(logits)


def two_calls(env, logits):
    env.step(env.sample_actions(logits)[0])


def with_torch(env, logits):
    d = torch.distributions.Categorical(logits=logits, validate_args=False)
    a = d.sample()
    env.torch_logp = d.log_prob(a)
    env.step(a.to(torch.uint8))


def sample(way, env, logits):
    """(us per call by device events, us per call of host enqueue time) over CALLS calls"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    h0 = time.perf_counter()
    for i in range(CALLS):
        way(env, logits[i % len(logits)])
    h1 = time.perf_counter()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / CALLS * 1e3, (h1 - h0) / CALLS * 1e6


A, B, C = "(a) step_sampled       ", "(b) sample, then step  ", "(c) torch, then step   "
WAYS = {A: fused, B: two_calls, C: with_torch}
say("tools/time_train_step_sample.py on one device: us per training step from policy logits [n, 2, 6] to the next observation, use_phi on, drawn starts, horizon 400;")
say("three envs in one process, alternating, %d samples of %d calls each after %d warm-up calls (device events); median (min..max), host = enqueue time of the same calls." % (REPEATS, CALLS, WARMUP))
say("(a) step_sampled: oc_multi_agent_step_sample; (b) sample_actions (oc_sample_actions), then step; (c) torch Categorical.sample + log_prob + cast to u8, then step (the way before).")
slower = []
for layout in layouts:
    for obs in ("ppo", "features"):
        for n in SIZES:
            kw = dict(horizon=400, reward_shaping_factor=1.0, device=dev, use_phi=True, random_start_pos=True, rnd_obj_prob_thresh=0.35, seed=0,
                      obs=obs, obs_dtype=torch.uint8)
            envs = {k: VecOvercookedMultiAgent(layout, n, **kw) for k in WAYS}
            logits = (torch.randn((16, n, 2, 6), device=dev) * 3.0).contiguous()
            plans = {A: envs[A].plan_sampled(), B: "k_sample_actions, then " + envs[B].plan(), C: "torch, then " + envs[C].plan()}
            assert "SAMPLE=true" in plans[A], plans
            for k, e in envs.items():
                for i in range(WARMUP):
                    WAYS[k](e, logits[i % len(logits)])
            times = {k: [] for k in envs}
            for _ in range(REPEATS):
                for k, e in envs.items():
                    times[k].append(sample(WAYS[k], e, logits))
            say("%s obs=%s n=%d" % (layout, obs, n))
            med, spread = {}, {}
            for k in envs:
                t = sorted(x[0] for x in times[k])
                h = sorted(x[1] for x in times[k])
                med[k], spread[k] = t[len(t) // 2], t[-1] - t[0]
                say("%s %7.2f us per call (min %.2f, max %.2f; host %.2f)   [%s]" % (k, med[k], t[0], t[-1], h[len(h) // 2], plans[k]))
            sp = max(spread[A], spread[B])
            keep = med[A] <= med[B] + sp
            if not keep:
                slower.append("%s obs=%s n=%d" % (layout, obs, n))
            say("    -> (a) - (b) = %+.2f us per call; larger spread of the two: %.2f us: %s.  (a) against (c): %.2f us, %.2fx"
                % (med[A] - med[B], sp, "fused stays the plan" if keep else "(a) IS SLOWER THAN (b) BY MORE THAN THE SPREAD", med[C] - med[A], med[C] / med[A]))
            del envs
say("shapes where (a) is slower than (b) by more than the spread: %s" % (", ".join(slower) if slower else "none"))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
