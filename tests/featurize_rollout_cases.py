"""One list of oc_rollout_featurize calls and the C oracle's run of such a call, one step at a time.

oc_rollout_featurize has two paths with identical results, chosen by plan_rollout_featurize (csrc/observation_plan.hpp): ONE kernel
instance, k_rollout_featurize<MAXP=2, FAST=3> (one two-player layout of at most 64 cells with one or two pots; `one_kernel`, or a
batch of at least 64 envs per CU and at least two steps), and the one-step entry points followed by oc_featurize, step by step.  Every
single-layout case below exists twice on the same inputs, `<id>` forced to the kernel and `<id>/steps` through the step-by-step
path; `expect` holds the words of oc_rollout_featurize_plan the case is there for.  tests/test_host_rollout_featurize.py holds the
list to the planner and shows on the oracle alone that each case contains what it claims; tests/test_gpu_rollout_featurize.py runs
every case against the oracle at zero tolerance.

Shapes, the smallest that can go wrong: 200 envs are one workgroup with a ragged fourth wavefront (8 envs: a quarter of an image),
321 envs a second workgroup of one full wavefront, one wavefront of one lane and two empty ones.  12 steps at horizon 8 with states
seeded over the whole horizon restart every env inside the launch, into drawn start states (DRAWN).  t0 = 5 with 1 and 3 steps starts
and ends a launch inside one Philox block (8 steps).

The features a row holds (featurize_state, mdp.py:2579-2898; csrc/featurize.hpp), own block first, per = num_pots * 10 + 26 wide:
  0..3 orientation, 4..7 held onion / soup / dish / tomato, 8..21 (dx, dy) of the closest onion, tomato, dish, soup (+ its onion and
  tomato counts at 16, 17), serving cell and empty counter, then per pot j at 22 + 10 j: exists, empty, full, cooking, ready, onions,
  tomatoes, cook time remaining, dx, dy, then four walls; the row ends with the other player's relative and this player's absolute
  position."""
import functools
from collections import namedtuple

import numpy as np

import derived_cases  # noqa: F401 (its tables — three_pots —: the import registers them)
import train_cases  # noqa: F401 (... and rollout_cases': mix5)
from case_support import DRAWN, caller_actions, layout_ids, new_oracle, register_grid, seeded_states, table_of

ONE_KERNEL = "k_rollout_featurize<MAXP=2, FAST=3>"
INSTANCES = (ONE_KERNEL,)  # every kernel instance csrc/observation_dispatch.hpp instantiates for oc_rollout_featurize
SEEDED = 4096              # a larger batch repeats the seeded states of its first 4 096 envs
N_BAD = 3                  # illegal actions per step of a call with caller actions
# 8 x 7 = 56 cells: four object planes, two pots, counters inside the room
EIGHT_BY_SEVEN = "XXPXXPXX\nO 1    X\nX      X\nX  XX  X\nD      X\nX    2 S\nXXXOXXXX"
register_grid("featurize_eight_by_seven", EIGHT_BY_SEVEN)

CALLS = ("random", "actions", "single_buffer")
Case = namedtuple("Case", "id table n_envs call one_kernel expect num_pots counter_goals n_steps horizon t0 start seed env_offset claims")
CASES = []


def step_by_step(entry, lay_lds=True):
    return "step by step: %s + k_featurize<LAY_LDS=%s>" % (entry, "true" if lay_lds else "false")


def total_of(num_pots):
    return 2 * (num_pots * 10 + 26) + 4


_POTS = {"cramped_room": 1, "cramped_room_old": 1, "cramped_room_tomato": 1, "asymmetric_advantages": 2, "featurize_eight_by_seven": 2}


def _claims(table, num_pots, counter_goals, n_steps):
    """What the case's run must contain, for both players (check_claims looks for each in the oracle's features): the pot classes of
    the closest pot and, on a two-pot layout, of the second; mixed tables and short launches claim no pot class."""
    if n_steps < 12:
        return ()
    out = ["restarts", "held_soup"] + ["counter_soup"] * (counter_goals == "all") + ["tomato_count"] * (table == "cramped_room_tomato")
    for j in range(min(num_pots, _POTS.get(table, 0))):
        out += ["pot%d_%s" % (j + 1, kind) for kind in ("empty", "idle_partly_full", "cooking", "ready")]
    return tuple(out)


def case(id, table, n_envs, call, num_pots, counter_goals, n_steps=12, horizon=8, t0=5, seed=7, env_offset=None, paths=(True, False)):
    """call: one of CALLS (random policy; caller actions with illegal entries; the random policy into one buffer that every step
    overwrites); paths: True = forced to the single kernel (`one_kernel`), False = step by step, under the id `<id>/steps`."""
    assert call in CALLS
    entry = "oc_step" if call == "actions" else "oc_rollout_random"
    for one in paths:
        k = len(CASES)
        CASES.append(Case(id + ("" if one else "/steps"), table, n_envs, call, one, ONE_KERNEL if one else step_by_step(entry), num_pots,
                          counter_goals, n_steps, horizon, t0, "drawn", seed, 3 * n_envs + 64 * (k // 2) + 37 if env_offset is None else env_offset,
                          _claims(table, num_pots, counter_goals, n_steps)))


# one pot, two object planes; the default num_pots = 2 leaves the second pot block zero
case("cramped_room_random", "cramped_room", 200, "random", 2, "none")
# two pots, three object planes, counters as goals, a second workgroup
case("asymmetric_counter_goals", "asymmetric_advantages", 321, "random", 2, "all")
# tomato counts; caller actions with illegal entries (flagged, the env untouched, its features recomputed unchanged)
case("tomato_actions", "cramped_room_tomato", 200, "actions", 2, "all")
# 56 cells: four object planes (16 object dwords in the counter walk); four pot blocks on a two-pot layout
case("four_planes_four_pots", "featurize_eight_by_seven", 321, "random", 4, "all")
# old dynamics (the other half of the interact table); no pot blocks at all: rows of 56 floats
case("old_dynamics_no_pots", "cramped_room_old", 200, "random", 0, "none")
case("asymmetric_actions_four_pots", "asymmetric_advantages", 200, "actions", 4, "none")
# stride 0: only the last step's features survive
case("single_buffer", "cramped_room", 321, "single_buffer", 2, "all")
# launches that start and end inside a Philox block
case("one_step_inside_a_block", "cramped_room", 200, "random", 2, "all", n_steps=1)
case("three_steps_inside_a_block", "cramped_room", 200, "random", 2, "all", n_steps=3)
# tables the single kernel does not take: five layouts; three pots — planned and run step by step, one_kernel or not
case("mix5_step_by_step", "mix5", 200, "random", 2, "all", paths=(False,))
case("three_pots_step_by_step_actions", "three_pots", 200, "actions", 4, "all", paths=(False,))
CASES = tuple(CASES)
assert len({c.id for c in CASES}) == len(CASES)

# The unforced default plan at the smallest batch the fill rule accepts (asked of the planner: 16 384 envs on 256 CUs): the run
# of the xcd_block mapping on a grid of 64 workgroups, eight per XCD
LAUNCH_SIZE = Case("launch_size_default_plan", "cramped_room", None, "random", False, ONE_KERNEL, 2, "none", 3, 8, 5, "drawn", 7, 1000, ())


def far_case():
    """A case at the far corner of the counter space (tests/far_cases.py): a seed with both halves set, an env offset whose low word
    wraps inside the batch, a t0 whose Philox block index wraps inside the launch (5 of the 12 steps below the wrap) and, with
    far_epoch0(), an epoch that wraps in the middle of the run — between two restarts of every env."""
    import far_cases as F

    c = next(c for c in CASES if c.id == "cramped_room_random")
    return c._replace(id="cramped_room_random@far", seed=F.FAR_SEED, env_offset=F.far_env_offset(c.n_envs), t0=F.FAR_T0_SHORT)


def far_epoch0(c):
    import far_cases as F

    return F.mid_epoch(c.n_steps)


def states_of(c):
    """uint8 [n_planes, n_envs, 16], read-only: the states the call starts from (computed once per case)"""
    c = c._replace(seed=c.seed & 0xFFFFFFFF)
    if c.n_envs <= SEEDED:
        return seeded_states(c)
    st = np.tile(seeded_states(c._replace(n_envs=SEEDED)), (1, -(-c.n_envs // SEEDED), 1))[:, :c.n_envs]  # (the streams are keyed by the env's index)
    st.setflags(write=False)
    return st


def actions_of(c):
    """uint8 [n_steps, n_envs, 2], read-only: the caller's actions, N_BAD illegal entries per step and one more at step 1; None for
    the random policy"""
    return caller_actions(c.n_steps, c.n_envs, N_BAD, c.seed & 0xFFFF) if c.call == "actions" else None


def env_kwargs(c):
    """Keyword arguments of the VecOvercookedEnv the case runs on (layouts, n_envs and device aside)."""
    return dict(horizon=c.horizon, layout_id=layout_ids(c), auto_reset=True, seed=c.seed, env_offset=c.env_offset, **DRAWN)


def plan_of_case(c, n_envs=None):
    """oc_rollout_featurize_plan's answer for the call the case makes (stand-in pointers)."""
    import ctypes

    from case_support import start_spec_of
    from overcooked_ai_amd import _lib, dispatch

    b = dispatch.batch_for(table_of(c.table), c.n_envs if n_envs is None else n_envs)
    start = start_spec_of(c)
    out = ctypes.create_string_buffer(320)
    rc = _lib.load().oc_rollout_featurize_plan(ctypes.byref(b), c.num_pots, c.horizon, _lib.OPT_AUTO_RESET | (_lib.OPT_ONE_KERNEL if c.one_kernel else 0),
                                               c.n_steps, int(c.call == "actions"), 1, ctypes.byref(start), out, len(out))
    _lib.check(rc, "oc_rollout_featurize_plan")
    return out.value.decode()


Trajectory = namedtuple("Trajectory", "rewards flags features state ep_returns")


@functools.lru_cache(maxsize=4)
def _trajectory(table, n_envs, call, num_pots, counter_goals, n_steps, horizon, t0, seed, env_offset, epoch0):
    from oracle import oracle as O

    c = Case("", table, n_envs, call, False, "", num_pots, counter_goals, n_steps, horizon, t0, "drawn", seed, env_offset, ())
    orc = new_oracle(table_of(table).specs)
    lid = layout_ids(c)
    state = states_of(c).copy()
    ep = np.zeros((n_envs, 4), np.float32)
    acts = actions_of(c)
    rewards, flags, feats = [], [], []
    for k in range(n_steps):
        start = O.start_spec(seed=seed, env_offset=env_offset, epoch=epoch0 + k, **DRAWN)
        kw = dict(horizon=horizon, options=1, layout_id=lid, ep_returns=ep, start=start)
        if acts is not None:
            state, rew, fl = orc.step(state, acts[k], **kw)
        else:
            rew, fl = orc.rollout_random(state, 1, seed=seed, env_offset=env_offset, t0=t0 + k, **kw)
            rew, fl = rew[0], fl[0]
        rewards.append(rew)
        flags.append(fl)
        feats.append(O.featurize(orc, state, counter_goals=counter_goals, num_pots=num_pots, layout_id=lid))
    out = Trajectory(np.stack(rewards), np.stack(flags), np.stack(feats), state, ep)
    for a in out:
        a.setflags(write=False)
    return out


def oracle_trajectory(c, epoch0=1):
    """The C oracle's run of the case, one step at a time — Oracle.step or Oracle.rollout_random(state, 1, t0 = t0 + k) with the start
    spec at epoch0 + k, then oracle.featurize —, computed once for the case's two paths: rewards [K, n, 4], flags [K, n], features
    [K, n, 2, total], the final states and episode returns; read-only.  epoch0: 1, a fresh env's first launch."""
    return _trajectory(c.table, c.n_envs, c.call, c.num_pots, c.counter_goals, c.n_steps, c.horizon, c.t0, c.seed, c.env_offset, epoch0)


def situations(c, traj):
    """claim -> per player, the (step, env) rows of the oracle's features that hold it (restarts: the count, for both)."""
    f = traj.features  # [K, n, 2, total]: row p starts with player p's own block
    held_soup = f[..., 5] == 1
    out = {"restarts": [int(((traj.flags & 4) != 0).sum())] * 2,
           "held_soup": held_soup.sum(axis=(0, 1)).tolist(),
           "counter_soup": (~held_soup & (f[..., 16] + f[..., 17] > 0)).sum(axis=(0, 1)).tolist(),
           "tomato_count": (f[..., 17] > 0).sum(axis=(0, 1)).tolist()}
    for j in range(min(c.num_pots, 2)):
        b = 22 + 10 * j
        exists, empty, full, cooking, ready = (f[..., b + i] == 1 for i in range(5))
        out["pot%d_empty" % (j + 1)] = (exists & empty).sum(axis=(0, 1)).tolist()
        out["pot%d_idle_partly_full" % (j + 1)] = (exists & ~empty & ~full & ~cooking & ~ready).sum(axis=(0, 1)).tolist()
        out["pot%d_cooking" % (j + 1)] = (exists & cooking & (f[..., b + 7] > 0)).sum(axis=(0, 1)).tolist()
        out["pot%d_ready" % (j + 1)] = (exists & ready).sum(axis=(0, 1)).tolist()
    return out


def check_claims(c, traj):
    """Every situation the case claims occurs for both players (restarts: at least n_envs of them): a quiet input cannot hide a
    failure.  Returns the counts."""
    found = situations(c, traj)
    for claim in c.claims:
        least = c.n_envs if claim == "restarts" else 1
        assert min(found[claim]) >= least, "%s claims %s and its run holds %s" % (c.id, claim, found[claim])
    return found
