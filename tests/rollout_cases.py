"""One list of oc_rollout_random calls, each there for ONE kernel instance, and the C oracle's run of such a call.

`oc_rollout_random` is not one kernel: choose_launch (csrc/rollout_dispatch.hpp) picks one of k_rollout4's non-recording instances
(R4Instances, csrc/shared.hpp) or one of k_rollout5's 24 from the table's hints, the batch size, the launch shape, the output
arrays, the event sink and two option bits.  Every case below names the instance it is there for (`expect`: the words of
oc_rollout_plan up to and including `>`); tests/test_host_rollout_instances.py holds the list to the planner's answers and to
the instances the sources list, without a GPU, and tests/test_gpu_launch_shapes.py runs every case against the oracle.

Unless a case is there for the standard start it has a nonzero env_offset, drawn start states (random_start_pos,
rnd_obj_prob_thresh 0.35: pots that arrive full, players that arrive holding soups) and at least two restarts per env inside
the launch (horizon < n_steps / 2)."""
import functools
from collections import namedtuple

import numpy as np

from case_support import DRAWN, EventCounts, layout_ids, new_oracle, register_table, table_of, tf as _tf  # noqa: F401 (DRAWN, table_of, layout_ids: for the tests)
from helpers import CANONICAL_5

PIPE_MAX = 98304       # envs up to which the one-wavefront instances read a step ahead (1.5 wavefronts per SIMD, 1 024 SIMDs)
N_LEAN = 131072 + 64   # above it, and not whole 256-env workgroups: the lean one-wavefront instances
N_RAGGED = 5000        # below it, not whole workgroups: the pipelined one-wavefront instances
N_WHOLE = 4096         # whole workgroups, one round: the mover / interact kernel
SEVEN = {"grid": "XPPPPPX\nO 1 2 O\nX     X\nXDPSPTX", "onion_time": 3, "tomato_time": 5, "onion_value": 7, "tomato_value": 4}
BIG_4 = ("marshmallow_experiment", "inverse_marshmallow_experiment", "marshmallow_experiment_coordination", "small_corridor")


def r4(UNIFORM=False, MAXP=8, LAY_LDS=False, MODE=0, OUT=False, OLD=True, EV=False, PIPE=True, RU=False, CW=2, NOCONF=False,
       FT8=False, REC=False):
    """A k_rollout4 instance in oc_rollout_plan's words; the defaults are R4Base's (csrc/shared.hpp)."""
    return ("k_rollout4<UNIFORM=%s, MAXP=%d, LAY_LDS=%s, MODE=%d, OUT=%s, OLD=%s, NF=%d, EV=%s, PIPE=%s, RU=%s, CW=%d, NOCONF=%s, "
            "FT8=%s, REC=%s>" % (_tf(UNIFORM), MAXP, _tf(LAY_LDS), MODE, _tf(OUT), _tf(OLD), 6 if MODE == 1 else 0, _tf(EV), _tf(PIPE),
                                 _tf(RU), CW, _tf(NOCONF), _tf(FT8), _tf(REC)))


def r5(LAY_LDS=True, FT8=False, OLD=False, BIG=False, EV=False, NOOUT=False):
    """A k_rollout5 instance in oc_rollout_plan's words."""
    return "k_rollout5<LAY_LDS=%s, FT8=%s, OLD=%s, BIG=%s, EV=%s%s>" % (_tf(LAY_LDS), _tf(FT8), _tf(OLD), _tf(BIG), _tf(EV),
                                                                         ", NOOUT=true" if NOOUT else "")


# the non-recording instances of R4Instances, by their names in csrc/shared.hpp, member by member as they are declared there
_J = dict(UNIFORM=True, LAY_LDS=True, OUT=True, OLD=False, MAXP=1, MODE=1)
_T = dict(OUT=True, OLD=False, MODE=2)
R4 = {
    "R4EvUniform": r4(UNIFORM=True, LAY_LDS=True, EV=True, MAXP=2),
    "R4EvSmall": r4(EV=True, MAXP=2),
    "R4EvGeneral": r4(EV=True),
    "R4JointTiled": r4(NOCONF=True, FT8=True, CW=4, **_J),
    "R4JointPipe": r4(NOCONF=True, CW=4, **_J),
    "R4JointLean": r4(PIPE=False, **_J),
    "R4TerrainUniform1": r4(UNIFORM=True, LAY_LDS=True, MAXP=1, CW=4, **_T),
    "R4TerrainUniform": r4(UNIFORM=True, LAY_LDS=True, MAXP=2, CW=4, **_T),
    "R4TerrainUniformLean": r4(UNIFORM=True, LAY_LDS=True, PIPE=False, MAXP=2, **_T),
    "R4TerrainLdsTiled": r4(LAY_LDS=True, RU=True, FT8=True, MAXP=2, CW=4, **_T),
    "R4TerrainLds": r4(LAY_LDS=True, RU=True, MAXP=2, CW=4, **_T),
    "R4TerrainLdsLean": r4(LAY_LDS=True, RU=True, PIPE=False, MAXP=2, **_T),
    "R4TerrainL2OnePotTiled": r4(RU=True, FT8=True, MAXP=1, CW=4, **_T),
    "R4TerrainL2OnePotLeanTiled": r4(RU=True, PIPE=False, FT8=True, MAXP=1, **_T),
    "R4TerrainL2OnePot": r4(RU=True, MAXP=1, CW=4, **_T),
    "R4TerrainL2OnePotLean": r4(RU=True, PIPE=False, MAXP=1, **_T),
    "R4TerrainL2": r4(RU=True, MAXP=2, CW=4, **_T),
    "R4TerrainL2Lean": r4(RU=True, PIPE=False, MAXP=2, **_T),
    "R4ArithUniformOut": r4(UNIFORM=True, LAY_LDS=True, OUT=True, OLD=False, MAXP=2),
    "R4ArithUniform": r4(UNIFORM=True, LAY_LDS=True, MAXP=2),
    "R4ArithLdsOut": r4(LAY_LDS=True, OUT=True, OLD=False, MAXP=2),
    "R4ArithL2Out": r4(OUT=True, OLD=False, MAXP=2),
    "R4ArithSmall": r4(MAXP=2),
    "R4ArithGeneral": r4(),
}
R4_NAME = {text: name for name, text in R4.items()}

Case = namedtuple("Case", "id table n_envs expect n_steps t0 horizon tiled one_wavefront outputs events start env_offset seed")


def case(id, table, n_envs, expect, n_steps=48, t0=0, horizon=20, tiled=False, one_wavefront=False, outputs=True, events=0,
         start="drawn", env_offset=None, seed=None):
    """outputs: both arrays or none; events: 0 no sink, 1 per-episode counters, 2 counters and per-step masks; start: "standard",
    "drawn" (DRAWN) or "regen" (drawn, and every restart re-draws the env's layout from the whole table)."""
    assert start in ("standard", "drawn", "regen") and events in (0, 1, 2)
    k = len(CASES)
    c = Case(id, table, n_envs, expect, n_steps, t0, horizon, tiled, one_wavefront, outputs, events, start,
             3 * n_envs + 64 * k if env_offset is None else env_offset, 11 + k if seed is None else seed)
    CASES.append(c)
    return c


CASES = []
# ---- k_rollout4: one wavefront per 64 envs.  Ragged batches (no whole workgroups) keep the mover / interact kernel away.
case("ev_uniform_masks", "coordination_ring", 2000, R4["R4EvUniform"], events=2)
case("ev_small_masks", "mix5", 2000, R4["R4EvSmall"], events=2)
case("ev_general_seven_pots", "seven_pots", 1000, R4["R4EvGeneral"], events=1)
case("joint_tiled", "cramped_room", N_RAGGED, R4["R4JointTiled"], tiled=True)
case("joint_pipe", "cramped_room", N_RAGGED, R4["R4JointPipe"])
case("joint_pipe_standard_start", "cramped_room", N_RAGGED, R4["R4JointPipe"], start="standard")
case("joint_lean", "cramped_room", N_LEAN, R4["R4JointLean"])
case("joint_pipe_whole_workgroups_one_wavefront", "cramped_room", N_WHOLE, R4["R4JointPipe"], one_wavefront=True)  # (the option bit)
case("joint_pipe_largest_ragged_batch", "cramped_room", PIPE_MAX - 64, R4["R4JointPipe"])
case("joint_lean_smallest_ragged_batch", "cramped_room", PIPE_MAX + 64, R4["R4JointLean"])
case("joint_lean_above_eight_rounds", "cramped_room", 8 * 65536 + 256, R4["R4JointLean"], n_steps=16, horizon=7)
case("joint_lean_shared_faces", "m_shaped_s", N_RAGGED, R4["R4JointLean"])  # (two players can face one cell: never pipelined)
case("terrain_uniform1", "scenario2_s", N_RAGGED, R4["R4TerrainUniform1"])
case("terrain_uniform", "asymmetric_advantages", N_RAGGED, R4["R4TerrainUniform"])
case("terrain_uniform_lean", "asymmetric_advantages", N_LEAN, R4["R4TerrainUniformLean"])
case("terrain_lds_tiled", "mix5", N_RAGGED, R4["R4TerrainLdsTiled"], tiled=True)
case("terrain_lds", "mix5", N_RAGGED, R4["R4TerrainLds"])
case("terrain_lds_lean", "mix5", N_LEAN, R4["R4TerrainLdsLean"])
case("terrain_l2_one_pot_tiled", "generated_4096", N_RAGGED, R4["R4TerrainL2OnePotTiled"], tiled=True)
case("terrain_l2_one_pot_lean_tiled", "generated_4096", N_LEAN, R4["R4TerrainL2OnePotLeanTiled"], tiled=True)
case("terrain_l2_one_pot", "generated_4096", N_RAGGED, R4["R4TerrainL2OnePot"])
case("terrain_l2_one_pot_regen", "generated_4096", N_RAGGED, R4["R4TerrainL2OnePot"], start="regen")
case("terrain_l2_one_pot_lean", "generated_4096", N_LEAN, R4["R4TerrainL2OnePotLean"])
case("terrain_l2_two_pots", "canonical_5_x8", N_RAGGED, R4["R4TerrainL2"])
case("terrain_l2_two_pots_lean", "canonical_5_x8", N_LEAN, R4["R4TerrainL2Lean"])
case("arith_uniform_out_65_cells", "marshmallow_experiment", N_RAGGED, R4["R4ArithUniformOut"])
case("arith_uniform_old", "cramped_room_old", N_RAGGED, R4["R4ArithUniform"])
case("arith_uniform_no_outputs", "asymmetric_advantages", N_RAGGED, R4["R4ArithUniform"], outputs=False)
case("arith_lds_out_65_cells", "big_4", N_RAGGED, R4["R4ArithLdsOut"])
case("arith_l2_out_65_cells", "big_4_x9", N_RAGGED, R4["R4ArithL2Out"])
case("arith_small_old", "canonical_4_old", N_RAGGED, R4["R4ArithSmall"])
case("arith_small_no_outputs", "mix5", N_RAGGED, R4["R4ArithSmall"], outputs=False)
case("arith_general_seven_pots", "seven_pots", 1000, R4["R4ArithGeneral"])
# ---- k_rollout5: mover + interact wavefronts, whole workgroups and whole 8-step blocks.  {table in LDS, through L2, 65..128
#      cells, event counters} x {new, old dynamics} x {tiled flags, [step][env] flags, no output arrays}
for _kind, _new, _old, _n, _kw in (("lds", "mix5", "canonical_4_old", N_WHOLE, dict()),
                                   ("l2", "canonical_5_x8", "canonical_4_old_x9", N_WHOLE, dict(LAY_LDS=False)),
                                   ("big", "big_4", "small_corridor_old", N_WHOLE, dict(BIG=True)),
                                   ("ev", "coordination_ring", "coordination_ring_old", 2048, dict(EV=True))):
    for _dyn, _table in (("new", _new), ("old", _old)):
        _o = dict(_kw, OLD=_dyn == "old")
        _ev = 1 if _kind == "ev" else 0
        case("duo_%s_%s_tiled" % (_kind, _dyn), _table, _n, r5(FT8=True, **_o), tiled=True, events=_ev)
        case("duo_%s_%s_flat" % (_kind, _dyn), _table, _n, r5(**_o), events=_ev)
        case("duo_%s_%s_no_outputs" % (_kind, _dyn), _table, _n, r5(NOOUT=True, **_o), outputs=False, events=_ev)
case("duo_l2_one_pot_regen", "generated_4096", N_WHOLE, r5(LAY_LDS=False), start="regen")
case("duo_lds_eight_rounds", "cramped_room", 8 * 65536, r5(), n_steps=16, horizon=7)  # (one workgroup per CU and round, 256 CUs)
case("duo_lds_two_rounds_standard_start", "cramped_room", 131072, r5(), start="standard")
# ---- a launch off the 8-step grid: head (5 steps) and tail (7) on the one-wavefront instances, the whole blocks between them
#      (288 steps) on the mover / interact kernel; the plan names the instance of the whole blocks
case("split_joint_table_layout", "cramped_room", N_WHOLE, r5(), n_steps=300, t0=3, horizon=100)
case("split_mix5_event_counters", "mix5", 2048, r5(EV=True), n_steps=300, t0=3, horizon=100, events=1)
CASES = tuple(CASES)
assert len({c.id for c in CASES}) == len(CASES)


def _composed(name):
    """The tables the cases name beside single registry layouts (case_support.table_of: those, and `<layout>_old`)."""
    from overcooked_ai_amd.layout_gen import reference_generated_layouts
    from overcooked_ai_amd.layouts import LayoutSpec, LayoutTable, spec_from_name

    old4 = CANONICAL_5[:4]  # (the canonical layouts whose orders all have three items: old dynamics accepts no others)
    if name == "mix5":
        return LayoutTable([spec_from_name(nm) for nm in CANONICAL_5], pad_to=(9, 5))
    if name == "canonical_5_x8":  # 40 layouts, two pots: more than LDS holds
        return LayoutTable([spec_from_name(nm) for nm in CANONICAL_5] * 8, pad_to=(9, 5))
    if name == "canonical_4_old":
        return LayoutTable([spec_from_name(nm, old_dynamics=True) for nm in old4], pad_to=(9, 5))
    if name == "canonical_4_old_x9":
        return LayoutTable([spec_from_name(nm, old_dynamics=True) for nm in old4] * 9, pad_to=(9, 5))
    if name == "big_4":  # 13 x 5 = 65 cells: 16-bit cell words, the 128-bit floor mask
        return LayoutTable([spec_from_name(nm) for nm in BIG_4])
    if name == "big_4_x9":
        return LayoutTable([spec_from_name(nm) for nm in BIG_4] * 9)
    if name == "generated_4096":
        return LayoutTable(reference_generated_layouts(4096))
    assert name == "seven_pots"
    return LayoutTable([LayoutSpec(SEVEN)])


for _name in ("mix5", "canonical_5_x8", "canonical_4_old", "canonical_4_old_x9", "big_4", "big_4_x9", "generated_4096", "seven_pots"):
    register_table(_name, functools.partial(_composed, _name))


def plan_of(table, n_envs, n_steps, t0, horizon, tiled=False, one_wavefront=False, outputs=True, events=0, start=None, regen=None,
            seed=0, env_offset=0, epoch=1, option=None):
    """oc_rollout_plan's answer for the call VecOvercookedEnv.rollout_random makes of these (auto_reset on; option: None, or the
    env's switch to an opt-in kernel, "lane_pair" / "predicate_interact")."""
    from overcooked_ai_amd import _lib, dispatch

    options = _lib.OPT_AUTO_RESET | (_lib.OPT_FLAGS_TILED8 if tiled else 0) | (_lib.OPT_ONE_WAVEFRONT if one_wavefront else 0)
    options |= {None: 0, "lane_pair": _lib.OPT_LANE_PAIR, "predicate_interact": _lib.OPT_PREDICATE_INTERACT}[option]
    sp = None
    if start or regen:
        first, count = regen or (0, 0)
        sp = _lib.OcStartSpec(seed, env_offset, epoch & 0xFFFFFFFF, int(bool((start or {}).get("random_start_pos"))),
                              float((start or {}).get("rnd_obj_prob_thresh", 0.0)), first, count)
    return dispatch.rollout_plan(table, n_envs, n_steps=n_steps, t0=t0, horizon=horizon, options=options, with_outputs=outputs,
                                 event_sink=events, start=sp)


def plan_of_case(c):
    table = table_of(c.table)
    return plan_of(table, c.n_envs, c.n_steps, c.t0, c.horizon, tiled=c.tiled, one_wavefront=c.one_wavefront, outputs=c.outputs,
                   events=c.events, start=None if c.start == "standard" else DRAWN,
                   regen=(0, len(table)) if c.start == "regen" else None, seed=c.seed, env_offset=c.env_offset)


class OracleLaunch:
    """The C oracle's run of one oc_rollout_random launch of a fresh VecOvercookedEnv (auto_reset): the first states (standard, or
    drawn at epoch 0 as the env's constructor draws them), then `chunks()` of steps.  `state`, `ep_returns`, `layout_id` and the
    event counters follow the launch in place.  start: None or the start_state_fn keywords; regen: None or (first, count);
    events: step by step, with the event_infos masks of every step and their per-episode counts, running and published."""

    def __init__(self, specs, n, layout_id=None, seed=0, env_offset=0, horizon=400, start=None, regen=None, events=False):
        from oracle import oracle as O

        self.O, self.orc = O, new_oracle(specs)
        self.n, self.seed, self.env_offset, self.horizon = n, seed, env_offset, horizon
        self.start, self.regen, self.events = dict(start or {}), regen, events
        self.layout_id = None if layout_id is None else np.ascontiguousarray(layout_id, dtype=np.uint16).copy()
        self.state = self.orc.reset(self.orc.new_state(n), layout_id=self.layout_id)
        if self.start:
            self.state = self.orc.reset_random(self.state, seed=seed, env_offset=env_offset, epoch=0, layout_id=self.layout_id,
                                               **self.start)
        self.ep_returns = np.zeros((n, 4), np.float32)
        self.event_counts = EventCounts(n)
        self.counts, self.counts_done = self.event_counts.running, self.event_counts.published

    def _spec(self, epoch):
        if not self.start and self.regen is None:
            return None
        return self.O.start_spec(seed=self.seed, env_offset=self.env_offset, epoch=epoch, regen=self.regen, **self.start)

    def chunks(self, n_steps, t0=0, epoch=1, chunk=400):
        """Yields (first step, rewards [k, n, 4], flags [k, n], event masks [k, n] u64 or None) for chunks of <= `chunk` steps —
        a 4 000-step launch of 131 072 envs does not fit the host's memory at once.  A restart at step j draws from epoch + j."""
        kw = dict(horizon=self.horizon, options=1, layout_id=self.layout_id, ep_returns=self.ep_returns)
        for c0 in range(0, n_steps, chunk):
            k = min(chunk, n_steps - c0)
            if not self.events:
                rew, fl = self.orc.rollout_random(self.state, k, seed=self.seed, env_offset=self.env_offset, t0=t0 + c0,
                                                  start=self._spec(epoch + c0), **kw)
                yield c0, rew, fl, None
                continue
            rew, fl = np.zeros((k, self.n, 4), np.float32), np.zeros((k, self.n), np.uint8)
            masks = np.zeros((k, self.n), np.uint64)
            for j in range(k):
                acts = self.O.random_actions(self.seed, self.env_offset, t0 + c0 + j, self.n)
                self.state, rew[j], fl[j] = self.orc.step(self.state, acts, start=self._spec(epoch + c0 + j), **kw)
                masks[j] = self.orc.last_events
                self.event_counts.update(masks[j], finished=(fl[j] & 1) != 0, cleared=(fl[j] & 4) != 0)  # (cleared at the restart)
            yield c0, rew, fl, masks


def oracle_launch_of(c):
    table = table_of(c.table)
    return OracleLaunch(table.specs, c.n_envs, layout_id=layout_ids(c), seed=c.seed, env_offset=c.env_offset, horizon=c.horizon,
                        start=None if c.start == "standard" else DRAWN, regen=(0, len(table)) if c.start == "regen" else None,
                        events=c.events > 0)
