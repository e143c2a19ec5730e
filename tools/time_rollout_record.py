"""Time recorded rollouts (oc_rollout_record: 400 fused steps storing every step's state and actions as well as rewards and
flags) for a layout / batch size, with the launch's rate and its share of the 8 TB/s HBM roofline on the recorded bytes:
    python tools/time_rollout_record.py [layout] [n_envs] [plain | events]
`plain`: the same launches through oc_rollout_random with OC_OPT_ONE_WAVEFRONT (no recording) for comparison.
`events`: oc_rollout_record_ex with every array — per-step event masks and layout ids too, per-episode event counters
(track_events).  layout `generated`: BASELINE configs[4]'s shape, the 4 096 generated terrains with a layout re-drawn at every
restart (regen_layout)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from overcooked_ai_amd.vec_env import VecOvercookedEnv

layout = sys.argv[1] if len(sys.argv) > 1 else "cramped_room"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
plain = "plain" in sys.argv[3:]
events = "events" in sys.argv[3:]
dev = torch.device("cuda:0")
if layout == "generated":
    from overcooked_ai_amd.layout_gen import reference_generated_layouts
    from overcooked_ai_amd.layouts import LayoutTable

    table = LayoutTable(reference_generated_layouts())
    env = VecOvercookedEnv(table, n, horizon=400, device=dev, auto_reset=True, seed=0,
                           layout_id=(np.arange(n) % len(table)).astype(np.uint16), regen_layout=True, track_events=events)
else:
    env = VecOvercookedEnv(layout, n, horizon=400, device=dev, auto_reset=True, seed=0, track_events=events)
env.one_wavefront = plain
T = 400
rew = torch.zeros((T, n, 4), dtype=torch.float32, device=dev)
fl = torch.zeros((T, n), dtype=torch.uint8, device=dev)
acts = None if plain else torch.zeros((T, n, 2), dtype=torch.uint8, device=dev)
states = None if plain else torch.zeros((T, env.n_planes, n, 16), dtype=torch.uint8, device=dev)
ev = torch.zeros((T, n), dtype=torch.int64, device=dev) if events else None
lids = torch.zeros((T, n), dtype=torch.int16, device=dev) if events else None


def launch():
    if plain:
        env.rollout_random(T, rew, fl)
    elif events:
        env.rollout_random(T, rew, fl, ev, actions_out=acts, states_out=states, layouts_out=lids)
    else:
        env.rollout_random(T, rew, fl, actions_out=acts, states_out=states)


for _ in range(5):
    launch()
torch.cuda.synchronize()
evs = [torch.cuda.Event(enable_timing=True) for _ in range(41)]
for i in range(40):
    evs[i].record()
    launch()
evs[40].record()
torch.cuda.synchronize()
ms = sorted(a.elapsed_time(b) for a, b in zip(evs[:-1], evs[1:]))
med = ms[len(ms) // 2]
# bytes written per env-step: rewards + flags, + the packed state and the actions, + the layout id and the event mask
per_step = 16 + 1 + (0 if plain else 16 * env.n_planes + 2) + (2 + 8 if events else 0)
rate = n * T / (med * 1e-3)
what = "one-wavefront oc_rollout_random" if plain else "oc_rollout_record_ex + events + layout ids" if events else "oc_rollout_record"
if layout == "generated":
    what += ", regen_layout"
print("%s n=%d %s: launch median %.1f us, min %.1f us -> %.3f us/step, %.1f G env-steps/s, %d B/env-step, %.2f TB/s = %.3f of 8 TB/s" % (
    layout, n, what, med * 1e3, ms[0] * 1e3, med * 1e3 / T, rate / 1e9, per_step, rate * per_step / 1e12, rate * per_step / 8e12))
