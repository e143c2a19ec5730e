"""One list of observation calls, each there for ONE kernel instance of the observation path, and the C oracle's run of such a call.

The observation path launches 13 kernel instances (csrc/observation_dispatch.hpp: launch_encode, launch_rollout_encode): k_encode_uniform<u8>,
k_encode<T, LAY_LDS> (4) and k_rollout_encode<MAXP=2, FAST, T, NW> (8).  plan_encode / plan_rollout_encode (csrc/
observation_plan.hpp) pick one from the table's hints, the batch size, the observation type and the option bits.  Every case below
names what it is there for (`expect`: the words of oc_observation_plan up to and including `>`, and those of unit=, G=, epb=,
upg=, grid= and the LDS bytes that the case is there for and that hold for any LDS budget from 147 456 to 160 000 bytes);
tests/test_host_observation_instances.py holds the list to the planner's answers and to the instances the sources instantiate,
without a GPU, and tests/test_gpu_observation_instances.py runs every case against the oracle at zero tolerance.

The rules the comments below re-derive the plans from are written out at the head of tests/test_host_observation_plan.py:
  env_bytes = 2 * cells * 26 * sizeof(T); unit = the fewest envs whose bytes are a multiple of 16; n_obj = ceil(cells / 16)
  k_encode           epb = 40960 // (env_bytes + 16 * (1 + n_obj)), a multiple of 4 when >= 4, at most 32; grid = ceil(n / epb)
  k_encode_uniform   upg = min(19 * env_bytes, 40960) // (unit * env_bytes), unit * upg <= 32; grid = ceil(n / (unit * upg))
                     LDS = unit * env_bytes * (1 + upg) + 16 * unit * upg * (1 + n_obj)
  k_rollout_encode   fixed = 8192 * n_obj + unit * env_bytes + 11520; gmax = (budget - fixed) // (8 * env_bytes); fewer than 4 (u8)
                     / 8 (f32): four wavefronts, gmax twice that; span = 32 / 64 envs in ceil(span / gmax) sub-groups of
                     G = ceil(span / parts) rounded up to unit (gmax rounded down to unit where that is more than gmax)

The states a call starts from are helpers.random_packed_states with timesteps over the whole horizon: a horizon of 60 puts a third
of the envs outside their last 40 steps (the urgency layer is mixed inside every wavefront) and 14 steps restart about a quarter of
them inside the launch.  Rollout cases set `one_kernel`; their restarts draw the start state (rollout_cases.DRAWN) unless the case
says "standard".  14 steps x 258 or 260 envs keep every row of a u8 trajectory a multiple of 16 bytes."""
import ctypes
from collections import namedtuple

import numpy as np

import train_cases  # noqa: F401 (its tables and rollout_cases': the import registers them)
from case_support import (DRAWN, caller_actions, instance_of, layout_ids, new_oracle, register_grid, seeded_states, start_spec_of,  # noqa: F401
                          table_of)

THIRDS = (0.95, 0.5, 0.05)  # counter fill of env e: THIRDS[e % 3] — crowded, half full and sparse envs side by side
LIST_CAP = 14               # RE_LIST_CAP (csrc/rollout_encode.hpp): an env with more objects sends its sub-group through the dword loop
N_BAD = 3                   # illegal actions per step of a call with caller actions
SIX_BY_FIVE = "XPXXPX\nO 1  O\nX   2X\nX    X\nXDXSXX"  # 30 cells = 2 mod 4: u8 rows of 1560 bytes = 8 mod 16, unit=2; two pots
# 32 cells (two object planes: the 8-slot object-dword loop), two pots, 15 counters: 17 places for an object, more than LIST_CAP
EIGHT_BY_FOUR = "XXPXXPXX\nO 1  2 X\nX      X\nXDXXXSXX"
SEVEN_BY_THREE = "XPXXPXX\nO1   2O\nXDXXSXX"  # 21 cells (odd: unit=4) small enough for images of three templates


def uniform(unit, upg, grid, lds=None):
    return "k_encode_uniform<T=u8> unit=%d, upg=%d, grid=%d" % (unit, upg, grid) + (", %d B LDS" % lds if lds else "")


def generic(T, lay_lds, epb=None, grid=None):
    text = "k_encode<T=%s, LAY_LDS=%s>" % (T, "true" if lay_lds else "false")
    return text + (" epb=%d" % epb if epb else "") + (", grid=%d" % grid if grid else "")


def single(FAST, T, NW, unit=None, G=None, lds=None):
    text = "k_rollout_encode<MAXP=2, FAST=%d, T=%s, NW=%d>" % (FAST, T, NW)
    return text + (" unit=%d" % unit if unit else "") + (", G=%d" % G if G else "") + (", %d B LDS" % lds if lds else "")


def step_by_step(entry, encode):
    return "step by step: %s + %s" % (entry, encode)


# Every kernel instance csrc/observation_dispatch.hpp instantiates for the observation path
INSTANCES = tuple([uniform(0, 0, 0).split(">")[0] + ">"] + [generic(t, ll) for t in ("u8", "f32") for ll in (True, False)]
                  + [single(f, t, w) for f in (3, 0) for t in ("u8", "f32") for w in (8, 4)])
_NO_U8_NW4 = ("four wavefronts need eight images of fewer than 4 envs (gmax < 4): the largest u8 grid the kernel takes, 48 cells, "
              "still holds (147456 - 38592) // (8 * 2496) = 5; no budget from 144 KiB up reaches it")
_NO_F32_NW8 = ("eight wavefronts need eight f32 images of >= 8 envs, which only a 9-cell grid gives (3x3: gmax 8; 4x3: 6); a 3x3 grid "
               "has one interior cell, cannot seat two players, and the oracle, like the reference (mdp.py:2389), encodes no "
               "one-player layout")
# Instances no call reaches without a tuning knob (OC_ROLLOUT_ENCODE_WAVES), each with its reason
UNREACHABLE = {single(3, "u8", 4): _NO_U8_NW4, single(0, "u8", 4): _NO_U8_NW4, single(3, "f32", 8): _NO_F32_NW8, single(0, "f32", 8): _NO_F32_NW8}

CALLS = ("encode", "rollout", "rollout_actions", "rollout_single_buffer", "step_encode")
Case = namedtuple("Case", "id table n_envs dtype call expect n_steps horizon t0 start fill seed env_offset hint")


def case(id, table, n_envs, dtype, call, expect, n_steps=None, horizon=60, t0=None, start=None, fill=None, seed=None, env_offset=None,
         hint=True):
    """dtype: "u8" / "f32"; call: one of CALLS (step_encode: n_steps calls of one step each); start: what a restart inside the call
    gives, "standard" or "drawn" (DRAWN); fill: None (random_packed_states' own 0 / 0.1 / 0.35 per env) or THIRDS; hint: False
    withholds OC_BATCH_TWO_PLAYERS."""
    assert call in CALLS and dtype in ("u8", "f32") and fill in (None, THIRDS)
    k = len(CASES)
    rollout = call != "encode"
    if start is None:  # (oc_step_encode takes the single kernel only without a start spec)
        start = "drawn" if call.startswith("rollout") else "standard"
    assert start in ("standard", "drawn")
    c = Case(id, table, n_envs, dtype, call, expect, (14 if rollout else 0) if n_steps is None else n_steps, horizon,
             (5 + k if call in ("rollout", "rollout_single_buffer") else 0) if t0 is None else t0, start, fill,
             41 + k if seed is None else seed, 3 * n_envs + 64 * k + 37 if env_offset is None else env_offset, hint)
    CASES.append(c)
    return c


CASES = []
# ---- k_encode_uniform<u8>: one layout, u8.  (5x4: env_bytes 1040, unit 1, upg 19760 // 1040 = 19)
# ceil(442 / 19) = 24 groups: a multiple of 8, the XCD mapping (three groups per XCD); the last group holds 442 - 23 * 19 = 5 envs
case("uniform_unit1_xcd_ragged", "cramped_room", 442, "u8", "encode", uniform(1, 19, 24))
# 5x5: env_bytes 1300 = 4 mod 16 -> unit 4, upg = 24700 // 5200 = 4: 17 groups of 16 envs, the last one of 1 env (1300 B: 81 chunks and a dword)
case("uniform_unit4_one_env_tail", "coordination_ring", 257, "u8", "encode", uniform(4, 4, 17))
# 14x9 = 126 cells = 2 mod 4: env_bytes 6552 = 8 mod 16 -> unit 2; upg = 40960 // 13104 = 3; 9 state planes:
# LDS = 13104 * 4 + 16 * 6 * 9 = 53280; ceil(99 / 6) = 17 groups, the last one of 3 envs (a unit and a half)
case("uniform_unit2_nine_planes", "corridor", 99, "u8", "encode", uniform(2, 3, 17, 53280), seed=41)  # (seeds named where the default leaves the ragged last group all urgent)
# 6x5: env_bytes 1560 = 8 mod 16 -> unit 2; upg = 29640 // 3120 = 9; ceil(67 / 18) = 4 groups, the last one of 13 envs
case("uniform_unit2_small", "six_by_five", 67, "u8", "encode", uniform(2, 9, 4))
# ---- k_encode<T, LAY_LDS>: (9x5 u8: epb = 40960 // (2340 + 64) = 17 -> 16; ceil(1001 / 16) = 63, the last block of 9 envs = 21060 B:
# 1316 chunks and a dword)
case("encode_u8_lds", "mix5", 1001, "u8", "encode", generic("u8", True, 16, 63))
case("encode_u8_l2", "canonical_5_x8", 1001, "u8", "encode", generic("u8", False, 16, 63))
# 13x5 = 65 cells, 6 planes: epb = 40960 // (3380 + 96) = 11 -> 8
case("encode_u8_65_cells", "big_4", 203, "u8", "encode", generic("u8", True, 8))
# 5x4 f32: epb = 40960 // (4160 + 48) = 9 -> 8; 9x5 f32: 40960 // (9360 + 64) = 4
case("encode_f32_lds", "cramped_room", 63, "f32", "encode", generic("f32", True, 8))
case("encode_f32_l2", "canonical_5_x8", 203, "f32", "encode", generic("f32", False, 4), seed=42)
# 10x6 f32: 40960 // (12480 + 80) = 3; 13x5 f32: 40960 // (13520 + 96) = 3 — blocks that are no multiple of 4 envs
case("encode_f32_epb3_one_layout", "scenario3", 100, "f32", "encode", generic("f32", True, 3))
case("encode_f32_epb3_four_layouts", "big_4", 100, "f32", "encode", generic("f32", True, 3))
# 14x9 f32: env_bytes 26208, epb = 40960 // (26208 + 144) = 1.  12 806 x 26 208 B = 335 619 648 > 320 MiB = 335 544 320: the
# streaming-store branch of k_encode (csrc/encode.hpp) within three envs of its smallest size
case("encode_f32_epb1_streamed", "corridor", 12806, "f32", "encode", generic("f32", True, 1, 12806))
# ---- k_rollout_encode<MAXP=2, FAST=3, T=u8, NW=8>
# 5x4: fixed = 8192 * 2 + 1040 + 11520 = 28944; gmax = 118512 // 8320 = 14 (15 from 153 744 bytes: three parts either way), G = 11
case("rollout_u8_unit1", "cramped_room", 260, "u8", "rollout", single(3, "u8", 8, 1, 11, 120464))
# 9x5: unit 4, fixed = 24576 + 9360 + 11520 = 45456; gmax = 102000 // 18720 = 5 (6): 7 (6) parts of 5 (6), up to the unit 8 > gmax -> 4
case("rollout_u8_unit4", "asymmetric_advantages", 260, "u8", "rollout", single(3, "u8", 8, 4, 4, 120336))
# 6x5: unit 2, n_obj 2, fixed = 16384 + 3120 + 11520 = 31024; gmax = 116432 // 12480 = 9 (10 from 155 824): 4 parts of 8;
# LDS = 31024 + 64 * 1560 = 130864.  258 = 4 * 64 + 2: the last wavefront holds one unit
case("rollout_u8_unit2", "six_by_five", 258, "u8", "rollout", single(3, "u8", 8, 2, 8, 130864))
# ... 257 envs (rows that are no multiple of 16 bytes: one buffer, overwritten every step) leave one env, half a unit, there
case("rollout_u8_unit2_single_buffer", "six_by_five", 257, "u8", "rollout_single_buffer", single(3, "u8", 8, 2, 8, 130864))
# 9x5 with every third env crowded: the list scatter and the 16-slot dword scatter (three object planes) in the same wavefront;
# 132 = 2 * 64 + 4 envs: rows of 132 * 2340 B are multiples of 16
case("rollout_u8_unit4_crowded", "asymmetric_advantages", 132, "u8", "rollout", single(3, "u8", 8, 4, 4), fill=THIRDS)
# 8x5: env_bytes 2080, unit 1, fixed = 24576 + 2080 + 11520 = 38176; gmax = 109280 // 16640 = 6 (7 from 154 656: five parts), G = 6 (7):
# the instance and the unit hold for any budget, G does not
case("rollout_u8_40_cells_crowded", "counter_circuit_o_1order", 260, "u8", "rollout", single(3, "u8", 8, 1), fill=THIRDS)
# 8x4: env_bytes 1664, unit 1, n_obj 2: fixed = 16384 + 1664 + 11520 = 29568; gmax = 117888 // 13312 = 8 (9 from 149 376): 4 parts of 8
case("rollout_u8_dword8", "eight_by_four", 260, "u8", "rollout", single(3, "u8", 8, 1, 8), fill=THIRDS, seed=58)
# ---- k_rollout_encode<MAXP=2, FAST=3, T=f32, NW=4>: eight f32 images of 8 envs fit no grid of two players (5x4: gmax =
# 113936 // 33280 = 3 < 8 -> four wavefronts, gmax 6..7); G follows the budget
case("rollout_f32_unit1", "cramped_room", 260, "f32", "rollout", single(3, "f32", 4, 1))
case("rollout_f32_45_cells", "asymmetric_advantages", 260, "f32", "rollout", single(3, "f32", 4, 1))
case("rollout_f32_nw4_two_pots", "cramped_room_two_pots", 260, "f32", "rollout", single(3, "f32", 4, 1))
case("rollout_f32_nw4_actions", "six_by_five", 258, "f32", "rollout_actions", single(3, "f32", 4, 1))
# ---- FAST=0: a two-player table whose caller withholds OC_BATCH_TWO_PLAYERS ("0 / unset is always safe", include/oc_amd.h)
case("rollout_fast0_u8", "cramped_room", 260, "u8", "rollout", single(0, "u8", 8, 1, 11, 120464), hint=False)
case("rollout_fast0_f32", "cramped_room", 260, "f32", "rollout", single(0, "f32", 4, 1), hint=False)
case("rollout_fast0_u8_actions_crowded", "asymmetric_advantages", 132, "u8", "rollout_actions", single(0, "u8", 8, 4, 4), fill=THIRDS, hint=False)
# ---- oc_step_encode with one_kernel: the single kernel with n_steps = 1 and caller actions, 14 calls
case("step_encode_one_kernel", "asymmetric_advantages", 260, "u8", "step_encode", single(3, "u8", 8, 4, 4))
# ---- step by step: tables the single kernel does not take (seven pots; five layouts), one_kernel or not
# 7x4: env_bytes 1456, unit 1, upg 19; ceil(1000 / 19) = 53 groups
case("rollout_step_by_step_seven_pots", "seven_pots", 1000, "u8", "rollout", step_by_step("oc_rollout_random", uniform(1, 19, 53)))
case("rollout_step_by_step_mix5_actions", "mix5", 1000, "f32", "rollout_actions", step_by_step("oc_step", generic("f32", True, 4, 250)))
# ---- k_rollout_encode<MAXP=2, FAST=3, T=u8, NW=8> once more (listed last: the seeds of the cases above follow their positions)
# 7x3: env_bytes 1092 = 4 mod 16 -> unit 4, n_obj 2, fixed = 16384 + 4368 + 11520 = 32272; gmax = 115184 // 8736 = 13 (14 from 154 576):
# 3 parts of ceil(32 / 3) = 11 envs, rounded UP to the unit: G = 12 (rounded down it would be 8) — images of three templates, sub-groups
# of 12, 12 and 8 envs per half wavefront; LDS = 32272 + 96 * 1092 = 137104
case("rollout_u8_unit4_three_templates", "seven_by_three", 260, "u8", "rollout", single(3, "u8", 8, 4, 12, 137104))
CASES = tuple(CASES)
assert len({c.id for c in CASES}) == len(CASES)
STREAMED = next(c for c in CASES if c.id == "encode_f32_epb1_streamed")


# this list's own tables
register_grid("six_by_five", SIX_BY_FIVE)
register_grid("eight_by_four", EIGHT_BY_FOUR)
register_grid("seven_by_three", SEVEN_BY_THREE)


def env_bytes(c):
    t = table_of(c.table)
    return 2 * t.width * t.height * 26 * (1 if c.dtype == "u8" else 4)


def states_of(c):
    """uint8 [n_planes, n_envs, 16], read-only: the states the call starts from (computed once per case)."""
    return seeded_states(c, counter_fill=c.fill)


def actions_of(c):
    """uint8 [n_steps, n_envs, 2], read-only: the caller's actions, N_BAD illegal entries (6, 89, 172) per step and one more at step
    1; None for the random policy."""
    return caller_actions(c.n_steps, c.n_envs, N_BAD, c.seed) if c.call in ("rollout_actions", "step_encode") else None


def n_illegal(c):
    return N_BAD * c.n_steps + 1


def plan_of_case(c):
    """oc_observation_plan's answer for the call the case makes (stand-in pointers; where the hint is withheld, the batch of
    dispatch.batch_for with OC_BATCH_TWO_PLAYERS cleared)."""
    from overcooked_ai_amd import _lib, dispatch

    code = _lib.OBS_U8 if c.dtype == "u8" else _lib.OBS_F32
    if c.call == "encode":
        return dispatch.observation_plan(table_of(c.table), c.n_envs, 0, code, horizon=c.horizon)
    start = start_spec_of(c)
    K = 1 if c.call == "step_encode" else c.n_steps
    options = _lib.OPT_AUTO_RESET | _lib.OPT_ONE_KERNEL
    b = dispatch.batch_for(table_of(c.table), c.n_envs)
    if not c.hint:
        b.batch_flags &= ~_lib.BATCH_TWO_PLAYERS & 0xFFFFFFFF
    out = ctypes.create_string_buffer(320)
    rc = _lib.load().oc_observation_plan(ctypes.byref(b), code, c.horizon, options, K, int(actions_of(c) is not None), 1,
                                         ctypes.byref(start) if start is not None else None, out, len(out))
    _lib.check(rc, "oc_observation_plan")
    return out.value.decode()


def group_envs(c, plan):
    """Envs the kernel encodes together: a sub-group of k_rollout_encode (G), a block of k_encode (epb), a group of k_encode_uniform
    (unit * upg) — read from the plan's text."""
    import re

    f = dict(re.findall(r"\b(unit|upg|epb|G)=(\d+)", plan))
    if "G" in f:
        return int(f["G"])
    return int(f["epb"]) if "epb" in f else int(f["unit"]) * int(f["upg"])


def env_kwargs(c):
    """Keyword arguments of the VecOvercookedEnv the case runs on (layouts, n_envs and device aside)."""
    from overcooked_ai_amd import _lib

    kw = dict(horizon=c.horizon, layout_id=layout_ids(c), auto_reset=c.call != "encode", seed=c.seed, env_offset=c.env_offset)
    if c.start == "drawn":
        kw.update(DRAWN)
    if not c.hint:
        kw["batch_flags_mask"] = ~_lib.BATCH_TWO_PLAYERS
    return kw


class OracleRun:
    """The C oracle's run of one case.  `state` and `ep_returns` follow the run in place; step(k) gives the rewards [n, 4] and
    flags [n] of step k (random policy: the Philox actions of step t0 + k; a restart at step k draws from epoch 1 + k, as a fresh
    VecOvercookedEnv's first launch does, or from epoch0 + k); obs(a, b) is the int32 lossless encoding of envs a..b-1 of the current
    states."""

    def __init__(self, c, epoch0=None):
        from oracle import oracle as O

        self.c, self.O, self.epoch0 = c, O, 1 if epoch0 is None else epoch0
        self.orc = new_oracle(table_of(c.table).specs)
        self.layout_id = layout_ids(c)
        self.state = states_of(c).copy()
        self.ep_returns = np.zeros((c.n_envs, 4), np.float32)
        self.actions = actions_of(c)

    def step(self, k):
        c = self.c
        start = self.O.start_spec(seed=c.seed, env_offset=c.env_offset, epoch=self.epoch0 + k, **DRAWN) if c.start == "drawn" else None
        kw = dict(horizon=c.horizon, options=1, layout_id=self.layout_id, ep_returns=self.ep_returns, start=start)
        if self.actions is not None:
            self.state, rew, fl = self.orc.step(self.state, self.actions[k], **kw)
            return rew, fl
        rew, fl = self.orc.rollout_random(self.state, 1, seed=c.seed, env_offset=c.env_offset, t0=c.t0 + k, **kw)
        return rew[0], fl[0]

    def obs(self, a=0, b=None):
        b = self.c.n_envs if b is None else b
        lid = None if self.layout_id is None else self.layout_id[a:b]
        return self.orc.encode_lossless(np.ascontiguousarray(self.state[:, a:b]), horizon=self.c.horizon, layout_id=lid)
