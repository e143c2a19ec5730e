"""One list of VecOvercookedMultiAgent.step runs with the featurize_state observation (obs="features" / "both"), each there for ONE
path of oc_multi_agent_step_featurize, and the reference of such a step.

oc_multi_agent_step_featurize has two paths with identical results, chosen by plan_train (csrc/train_dispatch.hpp): the
kernel k_train_step_feat<MAXP> (features without an observation array, one two-player layout of at most 64 cells with one or two
pots, no event sink; `one_kernel`, or a batch from the launch-size threshold on), and oc_multi_agent_step's own planned path followed by
k_featurize.  Every case names the words of oc_multi_agent_step_featurize_plan it is there for (`expect`, a prefix that ends with a
'>').  tests/test_host_train_featurize.py holds the list to the planner and to the instances the sources instantiate and shows on
the oracle alone that each case contains what it claims; tests/test_gpu_train_featurize.py steps every case beside
train_cases.OracleTrainStep + oracle.featurize at zero tolerance.

Defaults as in train_cases: 25 steps at horizon 11, drawn start states (DRAWN), a nonzero env offset, illegal actions on every step
of a batch of 127 envs or more (train_cases.actions_of); the smaller batches carry fewer (small_actions), so that every env still
restarts twice inside the run.  Shapes forced onto the kernel, the smallest at which it can go wrong: 1 env; 33 (one env past a
32-env image); 65 (one env of a second wavefront); 256 + 232 (a ragged last workgroup).

`claims`: what the oracle's run of the case must contain (test_host_train_featurize.py looks for each): "restarts" at least two per env,
"sparse" a nonzero sparse reward, "phi" a step that changes the potential, "illegal_last" illegal actions on the last step,
"features_move" an env whose features change between consecutive steps, "counter_object" (counter_goals="all") an object on a
counter that changes a feature against "none"."""
from collections import namedtuple

import numpy as np

import train_cases as TC
from case_support import layout_ids, start_spec_of, table_of

N_BAD = TC.N_BAD
GAMMA = TC.GAMMA
BASE_CLAIMS = ("restarts", "illegal_last", "features_move")


def feat_k(MAXP):
    """A k_train_step_feat instance in oc_multi_agent_step_featurize_plan's words."""
    return "k_train_step_feat<MAXP=%d>" % MAXP


def two_launches(step_plan, lay_lds=True, obs=False):
    """oc_multi_agent_step's own plan text (up to its '>' or, for the sequence, whole), then the featurize instance."""
    if step_plan.startswith("k_") and obs:
        step_plan += " + oc_encode_lossless"
    return "%s + k_featurize<LAY_LDS=%s>" % (step_plan, TC._tf(lay_lds))


INSTANCES = (feat_k(1), feat_k(2))  # every k_train_step_feat instance csrc/train_dispatch.hpp instantiates

Case = namedtuple("Case", "id table n_envs expect steps horizon obs obs_dtype use_phi factor start events env_offset seed num_pots "
                          "counter_goals one_kernel claims")
CASES = []


def case(id, table, n_envs, expect, steps=25, horizon=11, obs="features", obs_dtype=None, use_phi=True, factor=0.37, start="drawn",
         events=0, env_offset=None, seed=None, num_pots=2, counter_goals="none", one_kernel=True, claims=("sparse", "phi")):
    """obs: "features" or "both" (obs_dtype "u8" / "f32": the lossless observation's); claims: beside BASE_CLAIMS; the others as in
    train_cases.case."""
    assert start in ("standard", "drawn", "regen") and events in (0, 1) and obs in ("features", "both") and (obs == "both") == (obs_dtype is not None)
    k = len(CASES)
    claims = BASE_CLAIMS + tuple(c for c in claims if c != "phi" or use_phi) + (("counter_object",) if counter_goals == "all" else ())
    c = Case(id, table, n_envs, expect, steps, horizon, obs, obs_dtype, use_phi, factor, start, events,
             3 * n_envs + 64 * k + 37 if env_offset is None else env_offset, 41 + k if seed is None else seed, num_pots, counter_goals,
             one_kernel, claims)
    CASES.append(c)
    return c


RAGGED = 256 + 232
# ---- k_train_step_feat, forced with one_kernel: the smallest shapes at which it can go wrong
case("feat_one_env", "cramped_room", 1, feat_k(1), claims=())
case("feat_one_env_past_an_image_two_pots_counter_goals", "asymmetric_advantages", 33, feat_k(2), counter_goals="all", claims=("phi",))
case("feat_one_env_of_a_second_wavefront_one_pot_block", "coordination_ring", 65, feat_k(2), num_pots=1, counter_goals="all", claims=("phi",))
case("feat_ragged_last_workgroup_counter_goals", "cramped_room", RAGGED, feat_k(1), counter_goals="all")
case("feat_two_pots_ragged_last_workgroup", "asymmetric_advantages", RAGGED, feat_k(2))
case("feat_old_dynamics_no_pot_blocks", "cramped_room_old", 200, feat_k(1), num_pots=0)
case("feat_four_pot_blocks_smaller_images", "asymmetric_advantages", RAGGED, feat_k(2), num_pots=4, counter_goals="all")
case("feat_no_potential", "cramped_room", 65, feat_k(1), use_phi=False, claims=())
case("feat_annealed_factor", "coordination_ring", 200, feat_k(2), factor="anneal", counter_goals="all")
case("feat_standard_start", "cramped_room", 200, feat_k(1), start="standard", claims=("phi",))
# ---- oc_multi_agent_step's own path, then k_featurize
case("two_launches_both_u8", "cramped_room", 1000, two_launches(TC.step1(True, 1, True), obs=True), obs="both", obs_dtype="u8")
case("two_launches_both_f32", "asymmetric_advantages", 200, two_launches(TC.step1(True, 2, True), obs=True), obs="both", obs_dtype="f32",
     counter_goals="all")
case("two_launches_event_sink", "cramped_room", 200, two_launches(TC.step_k(True, True)), events=1)
case("two_launches_mix5_regen", "mix5", 300, two_launches(TC.step1(False, 2, True)), start="regen", counter_goals="all")
case("two_launches_65_cells", "marshmallow_experiment", 1500, two_launches(TC.step_k(True, False)))
case("two_launches_seven_pots_sequence", "seven_pots", 200, two_launches(TC.sequence(True, "drawn", obs=False)), num_pots=4)
case("two_launches_small_unforced_batch", "cramped_room", 200, two_launches(TC.step1(True, 1, True)), one_kernel=False)
CASES = tuple(CASES)
assert len({c.id for c in CASES}) == len(CASES)

# The unforced default plan at the smallest batch the launch-size threshold accepts (asked of the planner: fill_threshold()); a
# short run, still two restarts per env
DEFAULT_PLAN = Case("feat_default_plan_smallest_batch", "cramped_room", None, feat_k(1), 9, 4, "features", None, True, 0.37, "drawn", 0,
                    1000003, 97, 2, "none", False, BASE_CLAIMS + ("sparse", "phi"))


def far_case():
    """A case at the far corner of the counter space (tests/far_cases.py): a seed with both halves set and an env offset whose low
    word wraps inside the batch; with far_epoch0(), an epoch that wraps in the middle of the run."""
    import far_cases as F

    c = next(c for c in CASES if c.id == "feat_ragged_last_workgroup_counter_goals")
    return c._replace(id=c.id + "@far", seed=F.FAR_SEED, env_offset=F.far_env_offset(c.n_envs))


def far_epoch0(c):
    import far_cases as F

    return F.mid_epoch(c.steps)


def plan_of_case(c, n_envs=None):
    """oc_multi_agent_step_featurize_plan's answer for the call VecOvercookedMultiAgent.step makes of the case."""
    from overcooked_ai_amd import _lib, dispatch

    return dispatch.multi_agent_featurize_plan(
        table_of(c.table), c.n_envs if n_envs is None else n_envs, horizon=c.horizon, obs_dtype=_lib.OBS_U8 if c.obs_dtype == "u8" else _lib.OBS_F32,
        with_obs=c.obs == "both", num_pots=c.num_pots, options=_lib.OPT_ONE_KERNEL if c.one_kernel else 0, use_phi=c.use_phi,
        event_sink=c.events, start=start_spec_of(c))


def fill_threshold():
    """The smallest batch the default plan gives to the kernel (DEFAULT_PLAN's table and arrays), found by bisection on the planner."""
    lo, hi = 1, 1 << 22
    assert plan_of_case(DEFAULT_PLAN, hi).startswith("k_train_step_feat<") and not plan_of_case(DEFAULT_PLAN, lo).startswith("k_train_step_feat<")
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if plan_of_case(DEFAULT_PLAN, mid).startswith("k_train_step_feat<"):
            hi = mid
        else:
            lo = mid
    return hi


def default_plan_case():
    return DEFAULT_PLAN._replace(n_envs=fill_threshold())


def env_kwargs(c):
    """Keyword arguments of the VecOvercookedMultiAgent the case steps (layouts, n_envs, device and obs_dtype aside)."""
    kw = dict(horizon=c.horizon, use_phi=c.use_phi, gamma=GAMMA, seed=c.seed, env_offset=c.env_offset, layout_id=layout_ids(c),
              track_events=bool(c.events), obs=c.obs, num_pots=c.num_pots, counter_goals=c.counter_goals, one_kernel=c.one_kernel)
    kw.update(TC.ANNEAL if c.factor == "anneal" else dict(reward_shaping_factor=c.factor))
    if c.start != "standard":
        kw.update(TC.DRAWN)
    if c.start == "regen":
        kw["regen_layout"] = True
    return kw


def small_actions(c, t):
    """The actions of step t for a batch too small for train_cases.actions_of (fewer than 127 envs): the oracle's Philox draws with
    min(N_BAD, 2 * n_envs // steps) illegal ones per step, walking through the batch (an env loses at most three steps of the run to
    them, so it still restarts steps // horizon times), and one more for the batch's last env on the last step."""
    from oracle import oracle as O

    a = O.random_actions(c.seed, c.env_offset, t, c.n_envs)
    n_bad = min(N_BAD, 2 * c.n_envs // c.steps)
    for k in range(n_bad):
        a[(n_bad * t + k) % c.n_envs, (t + k) & 1] = 9
    if t == c.steps - 1:
        a[c.n_envs - 1, 0] = 9
    return a


def actions_of(c, t):
    """uint8 [n_envs, 2]: the actions of step t, illegal ones included (on the last step too)."""
    return TC.actions_of(c, t) if c.n_envs >= 127 else small_actions(c, t)


def features_of(c, ref, counter_goals=None):
    """float32 [n_envs, 2, total]: oracle.featurize of the states the reference's next step starts from."""
    f = ref.O.featurize(ref.orc, ref.state, counter_goals=c.counter_goals if counter_goals is None else counter_goals, num_pots=c.num_pots,
                        layout_id=ref.layout_id)
    return np.asarray(f, dtype=np.float32)


def total_of(num_pots):
    return 2 * (num_pots * 10 + 26) + 4
