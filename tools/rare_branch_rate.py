#!/usr/bin/env python
"""Where k_rollout5's rare-branch entries come from, counted on the C oracle (no GPU needed).

    python tools/rare_branch_rate.py [layout ...] [--envs 4096] [--steps 1200] [--horizon 400]

Random-policy rollouts from reset, envs grouped 64 to a wavefront as the kernel groups them.  Per layout: the share of wavefront-steps
in which some lane has a cooking start, a dish taken from the dispenser while the kernel's gate is open (N < 0 before or after
player 0's interact, N = 64 x loose dishes - useful pots: step_duo5.hpp), a delivery, the horizon; and the share with any of them,
a shared-cell replay (both players act on one cell and player 0 changes it: none on cramped_room, where no cell has two floor
neighbours); and the share with any of them, with and without cooking starts in the gate (the one-slot instances load a start's
countdown in the straight line).  causes() is the per-step census; tests/rare_path_cases.py counts its test launches with it."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import oracle as O  # noqa: E402
from overcooked_ai_amd import layouts  # noqa: E402


def hand_class(h):
    return np.where(h == 0, 0, np.where((h & 0x80) != 0, 4, np.minimum(h, 3)))


def pot_class(spec, o, tk):
    """0 empty, 1..3 idle with that many items, 4 cooking, 5 ready (arrays over envs)"""
    n = (o >> 3) & 3
    nt = np.array([bin(int(v) & 7).count("1") for v in o])
    cook = np.array([spec.recipe_time((int(a), int(b))) if a + b else 0 for a, b in zip(n - nt, nt)])
    return np.where(o == 0, 0, np.where(tk == 0, n, np.where(tk - 1 < cook, 4, 5)))


def causes(spec, st, nx, acts, fl):
    """One step of a batch on layout `spec` (packed states before / after, joint actions [n, 2], flag bytes) -> bool [n] per cause:
    start (a pot's tick byte leaves 0 without a restart), dish_gate (a dish taken from the dispenser while the kernel's gate is open),
    delivery, replay (both players act on one cell and player 0 changes it: player 1's interact is redone), horizon, restart."""
    n = st.shape[1]
    W = spec.width
    terrain = np.array([c for row in spec.terrain_mtx for c in row])
    pots = [y * W + x for x, y in spec.cells_of("P")]
    delta = np.array([-W, W, 1, -1])
    env = np.arange(n)
    obj = st[1:].transpose(1, 0, 2).reshape(n, -1)[:, :len(terrain)].astype(int)
    reset = (fl & 4) != 0
    pcs = [pot_class(spec, obj[:, p], st[0, :, 8 + k].astype(int)) for k, p in enumerate(pots)]
    useful = sum(((pc == 1) | (pc == 2) | (pc >= 4)).astype(int) for pc in pcs)
    N = 64 * (obj == 3).sum(axis=1) - useful
    face = [st[0, :, 3 * p].astype(int) + delta[st[0, :, 3 * p + 1] & 3] for p in (0, 1)]
    hand = [hand_class(st[0, :, 3 * p + 2].astype(int)) for p in (0, 1)]
    act = [acts[:, p] == 5 for p in (0, 1)]
    ter = [terrain[np.clip(f, 0, len(terrain) - 1)] for f in face]
    # player 0's change of N (lut5_entry: dn = 64 * dd - du) and whether it changes the cell it acts on (the entries' CHG flag)
    o0 = obj[env, np.clip(face[0], 0, len(terrain) - 1)]
    pc0 = np.zeros(n, int)
    for k, p in enumerate(pots):
        pc0 = np.where(face[0] == p, pcs[k], pc0)
    dn = np.zeros(n, int)
    on_x, on_p = act[0] & (ter[0] == "X"), act[0] & (ter[0] == "P")
    dn = np.where(on_x & (hand[0] == 0) & (o0 == 3), -64, dn)
    dn = np.where(on_x & (hand[0] == 3) & (o0 == 0), 64, dn)
    begins = on_p & (hand[0] == 0) & (pc0 >= 1) & (pc0 <= 3) & (not spec.old_dynamics)
    if not spec.old_dynamics:
        dn = np.where(on_p & (hand[0] == 0) & (pc0 == 3), -1, dn)
    dn = np.where(on_p & (hand[0] == 3) & (pc0 == 5), 1, dn)
    dn = np.where(on_p & ((hand[0] == 1) | (hand[0] == 2)) & (pc0 == 0), -1, dn)
    dn = np.where(on_p & ((hand[0] == 1) | (hand[0] == 2)) & (pc0 == 2), 1, dn)
    chg0 = (on_x & (((hand[0] == 0) & (o0 != 0)) | ((hand[0] != 0) & (o0 == 0)))) | begins | (on_p & (hand[0] == 3) & (pc0 == 5)) | \
           (on_p & ((hand[0] == 1) | (hand[0] == 2)) & (pc0 <= 2))
    take = (act[0] & (ter[0] == "D") & (hand[0] == 0)) | (act[1] & (ter[1] == "D") & (hand[1] == 0))
    return {"start": ((st[0, :, 8:8 + len(pots)] == 0) & (nx[0, :, 8:8 + len(pots)] != 0)).any(axis=1) & ~reset,
            "dish_gate": take & ((N < 0) | (N + dn < 0)),
            "delivery": (act[0] & (ter[0] == "S") & (hand[0] == 4)) | (act[1] & (ter[1] == "S") & (hand[1] == 4)),
            "replay": chg0 & act[1] & (face[1] == face[0]),
            "horizon": (fl & 1) != 0, "restart": reset}


def run(name, n, T, horizon):
    spec = layouts.spec_from_name(name)
    orc = O.Oracle([O.mdp_from_layout_dict(spec.to_layout_dict())])
    st = orc.reset(orc.new_state(n))
    ep = np.zeros((n, 4), np.float32)
    keys = ("start", "dish_gate", "delivery", "replay", "horizon", "any", "any_without_starts")
    cnt, lanes = dict.fromkeys(keys, 0), dict.fromkeys(keys, 0)
    for t in range(T):
        acts = O.random_actions(0, 0, t, n)
        nx, rew, fl = orc.step(st, acts, horizon=horizon, options=1, ep_returns=ep)
        m = causes(spec, st, nx, acts, fl)
        m["any_without_starts"] = m["dish_gate"] | m["delivery"] | m["replay"] | m["horizon"]
        m["any"] = m["any_without_starts"] | m["start"]
        for k in keys:
            cnt[k] += int(m[k].reshape(-1, 64).any(axis=1).sum())
            lanes[k] += int(m[k].sum())
        st = nx
    waves = (n // 64) * T
    print("%s: %d pot(s), %d envs x %d steps, horizon %d" % (name, len(spec.cells_of("P")), n, T, horizon))
    for k in keys:
        print("  %-20s %6.2f %% of wavefront-steps   %7.3f %% of env-steps" % (k, 100.0 * cnt[k] / waves, 100.0 * lanes[k] / (n * T)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("layouts", nargs="*", default=["cramped_room"])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--horizon", type=int, default=400)
    a = ap.parse_args()
    assert a.envs % 64 == 0
    for nm in a.layouts:
        run(nm, a.envs, a.steps, a.horizon)
