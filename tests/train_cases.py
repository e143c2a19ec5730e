"""One list of VecOvercookedMultiAgent.step runs, each there for ONE path or kernel instance of oc_multi_agent_step, and the plain
reference of such a step.

`oc_multi_agent_step` is not one kernel: plan_train (csrc/train_dispatch.hpp) picks k_train_step_obs<MAXP, T, NWV> (the step and
its observation in one kernel), k_train_step1<UNIFORM, MAXP, LAY_LDS> or k_train_step<UNIFORM, EV> (the step in one kernel, then
oc_encode_lossless), or the sequence of entry points, from the table's hints, the batch size, the observation array and its type
and the event sink.  Every case below names what it is there for (`expect`: the words of oc_multi_agent_plan up to and including
`>`; the whole text for the sequence); tests/test_host_train_instances.py holds the list to the planner's answers and to the
instances the sources instantiate, without a GPU, and tests/test_gpu_train_instances.py steps every case beside OracleTrainStep.

Unless a case is there for the standard start it has a nonzero env_offset, drawn start states (rollout_cases.DRAWN) and at least
two restarts per env inside the run (horizon < steps / 2).  The actions are the oracle's Philox draws (O.random_actions), uploaded;
a fixed handful per step is overwritten with 9, the illegal-action path: such an env stays untouched, timestep included, so
`steps % horizon` leaves room for it and every env still restarts steps // horizon times."""
from collections import namedtuple

import numpy as np

from case_support import DRAWN, EventCounts, layout_ids, new_oracle, register_grid, register_table, start_spec_of, table_of, tf as _tf
from rollout_cases import SEVEN  # (and its tables: the import registers them)

N_OBS = 32768           # the smallest batch k_train_step_obs serves: a workgroup of 256 envs for half of the 256 CUs (1 024 SIMDs / 8)
N_BAD = 5               # illegal actions per step
GAMMA = 0.99
# the annealed factor: 1.0 until step anneal_at() of the run (inside an episode), then what the reference's linear schedule gives
# for 337 of 1 000 timesteps, 1 - 337 / 1000 of the initial 1.0 — as a literal, so that the reference holds none of the product's Python
ANNEAL = dict(reward_shaping_factor=1.0, reward_shaping_horizon=1000)
ANNEAL_TIMESTEPS = 337
ANNEALED = 0.663


def obs_k(MAXP, T, NWV):
    """A k_train_step_obs instance in oc_multi_agent_plan's words."""
    return "k_train_step_obs<MAXP=%d, T=%s, NWV=%d>" % (MAXP, T, NWV)


def step1(UNIFORM, MAXP, LAY_LDS):
    return "k_train_step1<UNIFORM=%s, MAXP=%d, LAY_LDS=%s>" % (_tf(UNIFORM), MAXP, _tf(LAY_LDS))


def step_k(UNIFORM, EV):
    return "k_train_step<UNIFORM=%s, EV=%s>" % (_tf(UNIFORM), _tf(EV))


def sequence(use_phi, start, obs=True):
    """The sequence of entry points in oc_multi_agent_plan's words (both episode-return arrays are there)."""
    parts = ["oc_step"] + (["oc_potential"] if use_phi else []) + ["oc_shape_rewards", "copy of the episode returns"]
    parts += (["oc_regen_layouts"] if start == "regen" else []) + ["oc_reset" if start == "standard" else "oc_reset_random"]
    parts += (["oc_potential"] if use_phi and start != "standard" else []) + (["oc_encode_lossless"] if obs else [])
    return "sequence: " + ", ".join(parts)


# Every kernel instance csrc/train_dispatch.hpp instantiates for the training step; the sequence is a path, not an instance
INSTANCES = tuple([obs_k(p, t, w) for t in ("u8", "f32") for p in (1, 2) for w in (16, 8)]
                  + [step1(True, 1, True), step1(True, 2, True), step1(False, 2, True), step1(False, 2, False)]
                  + [step_k(u, ev) for u in (True, False) for ev in (True, False)])
# Instances no call reaches without a tuning knob, each with the condition of train_obs_shape that excludes it
UNREACHABLE = {obs_k(1, "f32", 16): "w == 16 && obs_dtype != OC_OBS_U8", obs_k(2, "f32", 16): "w == 16 && obs_dtype != OC_OBS_U8"}

Case = namedtuple("Case", "id table n_envs expect steps horizon obs use_phi factor start events env_offset seed")


def case(id, table, n_envs, expect, steps=25, horizon=11, obs="u8", use_phi=True, factor=0.37, start="drawn", events=0,
         env_offset=None, seed=None):
    """obs: "u8", "f32" or None (no observation array); factor: a number, or "anneal" (ANNEAL); start: "standard", "drawn" (DRAWN)
    or "regen" (drawn, and every restart re-draws the env's layout from the whole table); events: 1 = per-episode counters."""
    assert start in ("standard", "drawn", "regen") and events in (0, 1) and obs in ("u8", "f32", None)
    k = len(CASES)
    c = Case(id, table, n_envs, expect, steps, horizon, obs, use_phi, factor, start, events,
             3 * n_envs + 64 * k + 37 if env_offset is None else env_offset, 23 + k if seed is None else seed)
    CASES.append(c)
    return c


BIG = dict(steps=9, horizon=4)  # the batches of >= 32 767 envs: short runs, still two restarts per env
CASES = []
# ---- k_train_step_obs: the step and its observation in one kernel (single layout, <= 64 cells, >= N_OBS envs)
case("obs_one_pot_u8_16_waves_smallest_batch", "cramped_room", N_OBS, obs_k(1, "u8", 16), **BIG)
case("obs_one_pot_u8_16_waves_standard_start", "cramped_room", N_OBS, obs_k(1, "u8", 16), start="standard", **BIG)
case("obs_one_pot_u8_16_waves_old_dynamics", "cramped_room_old", N_OBS + 256, obs_k(1, "u8", 16), factor="anneal", **BIG)
case("obs_one_pot_u8_16_waves_four_rounds", "cramped_room", 131072 + 232 + 256, obs_k(1, "u8", 16), steps=7, horizon=3,
     env_offset=1000003)  # (a workgroup per CU and more; 232 envs in the last workgroup; an offset off the 256 grid)
case("obs_one_pot_u8_8_waves", "scenario2_s", N_OBS + 65, obs_k(1, "u8", 8), use_phi=False, **BIG)  # (65: one full wavefront and one env of the next)
case("obs_two_pots_u8_16_waves", "cramped_room_two_pots", N_OBS + 232, obs_k(2, "u8", 16), **BIG)
case("obs_two_pots_u8_8_waves", "asymmetric_advantages", N_OBS, obs_k(2, "u8", 8), factor="anneal", **BIG)
case("obs_two_pots_u8_8_waves_one_env_in_the_last_workgroup", "coordination_ring", N_OBS + 1, obs_k(2, "u8", 8), **BIG)  # (owners 1..3 idle)
case("obs_one_pot_f32_8_waves", "cramped_room", N_OBS + 1, obs_k(1, "f32", 8), obs="f32", use_phi=False, **BIG)
case("obs_two_pots_f32_8_waves", "coordination_ring", N_OBS + 65, obs_k(2, "f32", 8), obs="f32", **BIG)
# ---- k_train_step1: the step in one kernel on the wire format, then the observation kernel
case("step1_one_pot_largest_batch_below_the_switch", "cramped_room", N_OBS - 1, step1(True, 1, True), **BIG)
case("step1_one_pot_no_observation_array", "cramped_room", N_OBS + 232, step1(True, 1, True), obs=None, **BIG)
case("step1_two_pots_f32", "coordination_ring", 3000, step1(True, 2, True), obs="f32", factor="anneal")
case("step1_two_pots_standard_start", "asymmetric_advantages", 3000, step1(True, 2, True), start="standard")
case("step1_table_in_lds_regen", "mix5", 3000, step1(False, 2, True), start="regen")
case("step1_table_in_lds_regen_shaped", "mix5", 3000, step1(False, 2, True), start="regen", use_phi=False, obs="f32")
case("step1_table_through_l2_regen", "canonical_5_x8", 3000, step1(False, 2, False), start="regen")
case("step1_table_in_lds_old_dynamics", "canonical_4_old", 3000, step1(False, 2, True))
# ---- k_train_step: event counters, or 65..128 cells
case("step_events_one_layout", "cramped_room", 1500, step_k(True, True), events=1, use_phi=False)
case("step_events_mix5_regen", "mix5", 1500, step_k(False, True), events=1, start="regen")
case("step_65_cells_one_layout", "marshmallow_experiment", 3000, step_k(True, False), use_phi=False)
case("step_65_cells_table_regen", "big_4", 3000, step_k(False, False), start="regen")
# ---- the sequence of entry points: any other table (here: more than two pots)
case("sequence_seven_pots_drawn", "seven_pots", 1500, sequence(True, "drawn"))
case("sequence_seven_pots_standard_start", "seven_pots", 1500, sequence(True, "standard"), start="standard", obs="f32")
case("sequence_seven_pots_events_shaped", "seven_pots", 1500, sequence(False, "drawn"), events=1, use_phi=False, factor="anneal")
case("sequence_table_with_seven_pots_regen", "seven_and_scenario2_s", 3000, sequence(True, "regen"), start="regen")
# ---- old dynamics on k_train_step and on the sequence (k_train_step_obs and k_train_step1: above)
case("step_events_old_dynamics", "coordination_ring_old", 1500, step_k(True, True), events=1)
case("step_65_cells_old_dynamics", "small_corridor_old", 3000, step_k(True, False), factor="anneal")
case("sequence_three_pots_old_dynamics", "three_pots_old", 1500, sequence(True, "drawn"))
CASES = tuple(CASES)
assert len({c.id for c in CASES}) == len(CASES)


def _seven_and_scenario2_s():
    from overcooked_ai_amd.layouts import LayoutSpec, LayoutTable, spec_from_name

    return LayoutTable([LayoutSpec(SEVEN), spec_from_name("scenario2_s"), spec_from_name("cramped_room"),
                        table_of("cramped_room_two_pots").specs[0]], pad_to=(7, 4))


# this list's own tables, beside rollout_cases'
register_grid("cramped_room_two_pots", "XPPXX\nO  2O\nX1  X\nXDXSX")  # 20 cells, two pots: MAXP=2 with private images of >= 6 envs
# old dynamics accepts three-item orders only (not SEVEN's): cramped_room's, and three pots
register_grid("three_pots_old", "XPPPX\nO  2O\nX1  X\nXDXSX", old_dynamics=True)
# 7 x 4: a table with a layout of more than two pots (four layouts: a re-draw moves 3 envs of 4)
register_table("seven_and_scenario2_s", _seven_and_scenario2_s)


def factor_at(c, t):
    """reward_shaping_factor of step t of the run."""
    if c.factor != "anneal":
        return float(c.factor)
    return ANNEAL["reward_shaping_factor"] if t < anneal_at(c) else ANNEALED


def anneal_at(c):
    """The step before which an "anneal" case calls anneal_reward_shaping_factor(ANNEAL_TIMESTEPS): inside the second episode."""
    return c.horizon + 2


def actions_of(c, t):
    """uint8 [n_envs, 2]: the oracle's Philox actions of step t, N_BAD of them overwritten with 9 — envs no two steps share (so an
    env loses at most one step of its episodes to them), spread over the batch, and once its last env."""
    from oracle import oracle as O

    a = O.random_actions(c.seed, c.env_offset, t, c.n_envs)
    stride = (c.n_envs - 2) // (N_BAD * c.steps)
    assert stride >= 1
    for k in range(N_BAD):
        a[(N_BAD * t + k) * stride, (t + k) & 1] = 9
    if t == 1:
        a[c.n_envs - 1, 0] = 9
    return a


def plan_of_case(c):
    """oc_multi_agent_plan's answer for the call VecOvercookedMultiAgent.step makes of the case."""
    from overcooked_ai_amd import _lib, dispatch

    return dispatch.multi_agent_plan(table_of(c.table), c.n_envs, horizon=c.horizon, obs_dtype=_lib.OBS_F32 if c.obs == "f32" else _lib.OBS_U8,
                                     with_obs=c.obs is not None, use_phi=c.use_phi, event_sink=c.events, start=start_spec_of(c))


def env_kwargs(c):
    """Keyword arguments of the VecOvercookedMultiAgent the case steps (layouts, n_envs, device and obs_dtype aside)."""
    kw = dict(horizon=c.horizon, use_phi=c.use_phi, gamma=GAMMA, seed=c.seed, env_offset=c.env_offset, layout_id=layout_ids(c),
              track_events=bool(c.events), obs="ppo" if c.obs is not None else "bc")  # ("bc": step() gets no observation array)
    kw.update(ANNEAL if c.factor == "anneal" else dict(reward_shaping_factor=c.factor))
    if c.start != "standard":
        kw.update(DRAWN)
    if c.start == "regen":
        kw["regen_layout"] = True
    return kw


class OracleTrainStep:
    """The plain reference of VecOvercookedMultiAgent.step for a fresh env, from the C oracle's pieces and numpy float64 only:

        s', rewards, flags = orc.step(s, actions, options=0)       no auto-reset; an illegal action leaves the env untouched, flagged
        phi_next = O.potential(s')
        dense    = phi_next - phi_cur  (use_phi)  |  rewards[:, 2:4]
        shaped   = (rewards[:, 0] + rewards[:, 1]) + factor * dense     a product, then a sum: two roundings
        done     = flags & 1;  ep_out = the episode returns before the restart
        done envs: (regen: a new layout,) the drawn state of this step's epoch or the standard start state; returns cleared
        phi_cur  = phi_next; where done: phi_start[layout] (standard start) | O.potential of the drawn state on the new layout

    `state`, `ep_returns`, `layout_id`, `phi_cur` and the event counters follow the run in place; every other attribute is that of
    the last step.  Epoch 0 belongs to the constructor's states, step t draws from epoch 1 + t."""

    def __init__(self, specs, n, layout_id=None, seed=0, env_offset=0, horizon=400, start=None, regen=None, use_phi=True, events=False,
                 gamma=GAMMA):
        from oracle import oracle as O
        from overcooked_ai_amd.potential import potential_params

        self.O, self.orc = O, new_oracle(specs)
        self.n, self.seed, self.env_offset, self.horizon = n, seed, env_offset, horizon
        self.start, self.regen, self.use_phi, self.events = dict(start or {}), regen, use_phi, events
        self.layout_id = None if layout_id is None else np.ascontiguousarray(layout_id, dtype=np.uint16).copy()
        self.state = self.orc.reset(self.orc.new_state(n), layout_id=self.layout_id)
        if self.start:
            self.state = self.orc.reset_random(self.state, seed=seed, env_offset=env_offset, epoch=0, layout_id=self.layout_id, **self.start)
        self.epoch = 1
        self.ep_returns = np.zeros((n, 4), np.float32)
        self.event_counts = EventCounts(n)
        self.counts, self.counts_done = self.event_counts.running, self.event_counts.published
        self.phi_cur = self.phi_next = np.zeros((n,), np.float64)
        if use_phi:
            L = len(specs)
            self.params = [potential_params(s, gamma) for s in specs]
            every = None if L == 1 else np.arange(L, dtype=np.uint16)
            self.phi_start = O.potential(self.orc, self.orc.reset(self.orc.new_state(L), layout_id=every), self.params, layout_id=every)
            self.phi_cur = self._phi(self.state)

    def _phi(self, state):
        return self.O.potential(self.orc, state, self.params, layout_id=self.layout_id)

    def step(self, actions, factor):
        O, orc = self.O, self.orc
        self.state, self.rewards, self.flags = orc.step(self.state, actions, horizon=self.horizon, options=0, layout_id=self.layout_id,
                                                        ep_returns=self.ep_returns)
        r64 = self.rewards.astype(np.float64)
        if self.use_phi:
            self.phi_next = self._phi(self.state)
            self.dense = np.repeat((self.phi_next - self.phi_cur)[:, None], 2, axis=1)
        else:
            self.dense = r64[:, 2:4].copy()
        product = np.float64(factor) * self.dense
        self.shaped = (r64[:, 0] + r64[:, 1])[:, None] + product
        self.done = (self.flags & 1).astype(np.uint8)
        fin = self.done != 0
        self.ep_out = self.ep_returns.copy()
        if self.events:
            self.event_counts.update(orc.last_events, finished=fin, cleared=fin)  # (no auto-reset here: cleared where done)
        if self.start or self.regen is not None:
            spec = O.start_spec(seed=self.seed, env_offset=self.env_offset, epoch=self.epoch, regen=self.regen, **self.start)
            if self.regen is not None and self.layout_id is not None:
                O.regen_layouts(self.layout_id, spec, mask=self.done)
            self.state = orc.reset_random(self.state, seed=self.seed, env_offset=self.env_offset, epoch=self.epoch, layout_id=self.layout_id,
                                          mask=self.done, **self.start)
            self.ep_returns[fin] = 0
            if self.use_phi:
                self.phi_cur = np.where(fin, self._phi(self.state), self.phi_next)
        else:
            self.state = orc.reset(self.state, layout_id=self.layout_id, mask=self.done, ep_returns=self.ep_returns)
            if self.use_phi:
                lid = np.zeros((self.n,), np.int64) if self.layout_id is None else self.layout_id.astype(np.int64)
                self.phi_cur = np.where(fin, self.phi_start[lid], self.phi_next)
        self.epoch += 1
        return self

    def obs(self, a, b):
        """int32 [b - a, 2, W, H, 26]: the lossless encoding of envs a..b-1 of the states the next step starts from."""
        lid = None if self.layout_id is None else self.layout_id[a:b]
        return self.orc.encode_lossless(np.ascontiguousarray(self.state[:, a:b]), horizon=self.horizon, layout_id=lid)


def oracle_of(c):
    table = table_of(c.table)
    return OracleTrainStep(table.specs, c.n_envs, layout_id=layout_ids(c), seed=c.seed, env_offset=c.env_offset, horizon=c.horizon,
                           start=None if c.start == "standard" else DRAWN, regen=(0, len(table)) if c.start == "regen" else None,
                           use_phi=c.use_phi, events=c.events > 0)
