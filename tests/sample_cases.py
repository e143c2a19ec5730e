"""One list of VecOvercookedMultiAgent.step_sampled runs, each there for ONE path of oc_multi_agent_step_sample, the sampler of
include/oc_amd.h (OcActionSampler) restated twice in numpy, and the logits of every (case, step).

oc_multi_agent_step_sample draws both players' actions from policy logits and steps.  Wherever the same call with an actions array
is planned as k_train_step_obs, k_train_step_feat or k_train_step1, the SAMPLE = true instance of that kernel draws the actions
itself (one launch); every other plan runs k_sample_actions in front of the step's own path (csrc/train_dispatch.hpp).  Every case names
the words of oc_multi_agent_step_sample_plan it is there for (`expect`, a prefix that ends with a '>' or, for the sequence, with its
first words).  tests/test_host_train_sample.py holds the list to the planner and to the instances the sources instantiate and shows
on the references alone that each case contains what it claims; tests/test_gpu_train_sample.py steps every case.

The sampler, restated: `uniforms` (a vectorised numpy Philox on the header's counters), `sample_f32` (the header's arithmetic, step
by step in float32) and `sample_f64` (softmax and cumulative sums in float64, with the same u_p).  The two agree except where u * S
falls within rounding of a cumulative sum; `sample_f64` also returns that boundary band, |u * S - c_i| <= 2^-18 * S for some i.  The
float32 error of a c_i is at most about 6 * 2^-23 * S (six roundings of expf, five of the sums), so the band has about five times
margin; it holds about 2e-5 of the samples, and a case may have at most BAND_CAP of its samples in it.

Logits of (case, step): a seeded numpy generator, normal times 3, about 10 % of the entries -inf (never a whole row), and on batches
of at least 127 envs N_BAD rows with a NaN on every step, the last included (invalid rows: action 255, logp NaN, the env flagged
OC_F_BAD_ACTION and untouched) — rows no two steps share, so that every env still restarts steps // horizon times.

Defaults as in train_cases: 25 steps at horizon 11, drawn start states, a nonzero env offset; the batches of k_train_step_obs
(>= train_cases.N_OBS envs) 9 steps at horizon 4.

`claims`: what the reference's run of the case must contain: "restarts" at least two per env, "all_actions" every action 0..5 drawn
for both players, "masked" a -inf entry in the logits (and never drawn), "nan_last" an invalid row on the last step, "sparse" a
nonzero sparse reward."""
from collections import namedtuple

import numpy as np

import train_cases as TC
from case_support import DRAWN, layout_ids, start_spec_of, table_of  # noqa: F401

N_OBS = TC.N_OBS
N_BAD = TC.N_BAD
GAMMA = TC.GAMMA
BAND = 2.0 ** -18     # the boundary band, relative to S
BAND_CAP = 1e-3       # the share of a case's samples that may lie in it
LOGP_TOL = 1e-5       # |logp - float64 reference| on the drawn action: |l - m| < 32 and |logp| < 32 in the tested range, where one
#                       f32 ulp is at most 1.9e-6; a few roundings (l - m, expf, the sums, logf, the difference) sit on top
KEY_TWEAK = 0x53414D50  # "SAMP"
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------ the stream
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) on uint32 arrays (or scalars) of one shape -> the four output words, uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(x).astype(np.uint64) & M32 for x in np.broadcast_arrays(c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return tuple(x.astype(np.uint32) for x in (c0, c1, c2, c3))


def uniforms(seed, env_offset, step, n, drop=None):
    """float32 [n, 2]: u_p of envs 0..n-1 at the caller's step counter `step`.  drop: None, or one part of the counters a kernel could
    lose — "t_hi", "g_hi", "carry" (g_hi taken from env_offset alone), "tweak" (seed_hi without the key's "SAMP")."""
    assert drop in (None, "t_hi", "g_hi", "carry", "tweak")
    seed, step = int(seed) & (2**64 - 1), int(step) & (2**64 - 1)
    g = np.uint64(int(env_offset) & (2**64 - 1)) + np.arange(n, dtype=np.uint64)
    g_lo, g_hi = g & M32, g >> np.uint64(32)
    if drop == "g_hi":
        g_hi = np.zeros_like(g_hi)
    if drop == "carry":
        g_hi = np.full_like(g_hi, (int(env_offset) & (2**64 - 1)) >> 32)
    t_lo, t_hi = step & 0xFFFFFFFF, 0 if drop == "t_hi" else step >> 32
    k1 = (seed >> 32) ^ (0 if drop == "tweak" else KEY_TWEAK)
    r = philox4x32_10(np.full(n, t_lo, np.uint64), g_lo, g_hi, np.full(n, t_hi, np.uint64), seed & 0xFFFFFFFF, k1)
    u = np.stack([r[0] >> np.uint32(8), r[1] >> np.uint32(8)], axis=1).astype(np.float32) * np.float32(2.0 ** -24)
    return u


# ------------------------------------------------------------------------------------------ the sampler, twice
def _sample(logits, u, greedy, ft):
    """The header's arithmetic in the float type ft -> (actions int64 [n, 2], logp ft [n, 2], c ft [n, 2, 6], x ft [n, 2])"""
    l = np.asarray(logits, dtype=np.float32).astype(ft)
    with np.errstate(all="ignore"):
        nan = np.isnan(l).any(axis=-1)
        m = np.where(nan, ft(0), np.max(np.where(np.isnan(l), ft(-np.inf), l), axis=-1))
        w = np.exp((l - m[..., None]).astype(ft)).astype(ft)
        c = np.empty_like(w)
        acc = np.zeros(l.shape[:-1], ft)
        for i in range(6):
            acc = (acc + w[..., i]).astype(ft)
            c[..., i] = acc
        S = c[..., 5]
        bad = nan | ~(np.isfinite(S) & (S > 0))
        x = (np.asarray(u, dtype=np.float32).astype(ft) * S).astype(ft)
        if greedy:
            a = np.argmax(l == m[..., None], axis=-1)
        else:
            a = np.minimum((c <= x[..., None]).sum(axis=-1), 5)
        la = np.take_along_axis(l, a[..., None], axis=-1)[..., 0]
        logp = ((la - m).astype(ft) - np.log(S).astype(ft)).astype(ft)
    a = np.where(bad, 255, a).astype(np.int64)
    logp = np.where(bad, ft(np.nan), logp).astype(ft)
    return a, logp, c, x


def sample_f32(logits, u, greedy=False):
    """The float32 restatement -> (actions uint8 [n, 2], logp float32 [n, 2])"""
    a, logp, _, _ = _sample(logits, u, greedy, np.float32)
    return a.astype(np.uint8), logp


def sample_f64(logits, u, greedy=False):
    """The float64 reference -> (actions uint8 [n, 2], logp float64 [n, 2], band bool [n, 2]: u * S within BAND * S of a cumulative
    sum, where float32 arithmetic may draw the neighbouring action; never for greedy or invalid rows)"""
    a, logp, c, x = _sample(logits, u, greedy, np.float64)
    with np.errstate(all="ignore"):
        band = (np.abs(x[..., None] - c) <= BAND * c[..., 5:6]).any(axis=-1) & (a != 255) & (not greedy)
    return a.astype(np.uint8), logp, band


def logp_f64(logits, actions):
    """float64 [n, 2]: the reference's log-probability of `actions` (uint8 [n, 2], none of them 255) under `logits`."""
    l = np.asarray(logits, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        m = l.max(axis=-1)
        S = np.exp(l - m[..., None]).cumsum(axis=-1)[..., 5]
        la = np.take_along_axis(l, np.asarray(actions).astype(np.int64)[..., None], axis=-1)[..., 0]
        return (la - m) - np.log(S)


# ------------------------------------------------------------------------------------------ the cases
def _sampled(text):
    """A step kernel instance in oc_multi_agent_step_sample_plan's words: SAMPLE=true as its last parameter."""
    assert text.endswith(">")
    return text[:-1] + ", SAMPLE=true>"


def obs_k(MAXP, T, NWV):
    return _sampled(TC.obs_k(MAXP, T, NWV))


def step1(UNIFORM, MAXP, LAY_LDS):
    return _sampled(TC.step1(UNIFORM, MAXP, LAY_LDS))


def feat_k(MAXP):
    return _sampled("k_train_step_feat<MAXP=%d>" % MAXP)


def unfused(step_plan):
    return "k_sample_actions + " + step_plan


# Every SAMPLE = true instance csrc/train_dispatch.hpp instantiates
INSTANCES = tuple([obs_k(p, t, w) for t in ("u8", "f32") for p in (1, 2) for w in (16, 8)]
                  + [step1(True, 1, True), step1(True, 2, True), step1(False, 2, True), step1(False, 2, False)] + [feat_k(1), feat_k(2)])
# Instances no call reaches without a tuning knob, each with the condition of train_obs_shape (csrc/train_dispatch.hpp) that excludes it
UNREACHABLE = {obs_k(1, "f32", 16): "w == 16 && obs_dtype != OC_OBS_U8", obs_k(2, "f32", 16): "w == 16 && obs_dtype != OC_OBS_U8"}

Case = namedtuple("Case", "id table n_envs expect steps horizon obs use_phi factor start events env_offset seed one_kernel greedy step0 "
                          "num_pots counter_goals claims")
CASES = []
BASE_CLAIMS = ("restarts", "masked")


def case(id, table, n_envs, expect, steps=25, horizon=11, obs="u8", use_phi=True, factor=0.37, start="drawn", events=0, env_offset=None,
         seed=None, one_kernel=False, greedy=False, step0=0, claims=("all_actions", "sparse")):
    """obs: "u8" / "f32" (the lossless observation, obs="ppo"), None (no observation array) or "features" (featurize_state, with
    one_kernel: k_train_step_feat whatever the batch size); greedy: argmax mode; step0: the env's sample counter before the first
    step; claims: beside BASE_CLAIMS (and "nan_last" on batches of at least 127 envs); the others as in train_cases.case."""
    assert start in ("standard", "drawn", "regen") and events in (0, 1) and obs in ("u8", "f32", None, "features")
    k = len(CASES)
    claims = BASE_CLAIMS + tuple(claims) + (("nan_last",) if n_envs >= 127 else ())
    c = Case(id, table, n_envs, expect, steps, horizon, obs, use_phi, factor, start, events,
             3 * n_envs + 64 * k + 37 if env_offset is None else env_offset, 61 + k if seed is None else seed, one_kernel, greedy, step0,
             2, "none", claims)
    CASES.append(c)
    return c


RAGGED = 256 + 232
BIG = dict(steps=9, horizon=4)
FEAT = dict(obs="features", one_kernel=True)
# ---- fused, k_train_step_feat (forced with one_kernel) and k_train_step1 (obs "ppo" below the switch, or no observation array):
#      the smallest shapes at which they can go wrong
case("feat_one_env", "cramped_room", 1, feat_k(1), claims=(), **FEAT)
case("feat_one_env_past_an_image_two_pots", "asymmetric_advantages", 33, feat_k(2), claims=("all_actions",), **FEAT)
case("feat_one_env_of_a_second_wavefront_no_potential", "cramped_room", 65, feat_k(1), use_phi=False, claims=("all_actions",), **FEAT)
case("feat_ragged_last_workgroup", "cramped_room", RAGGED, feat_k(1), **FEAT)
case("feat_two_pots_ragged_last_workgroup", "coordination_ring", RAGGED, feat_k(2), claims=("all_actions",), **FEAT)
case("step1_one_env_u8", "cramped_room", 1, step1(True, 1, True), claims=())
case("step1_one_env_of_a_second_wavefront_f32", "asymmetric_advantages", 65, step1(True, 2, True), obs="f32", claims=("all_actions",))
case("step1_ragged_last_workgroup_old_dynamics", "cramped_room_old", RAGGED, step1(True, 1, True), obs=None)
case("step1_mix5_regen", "mix5", 300, step1(False, 2, True), start="regen")
case("step1_table_through_l2_regen_no_potential", "canonical_5_x8", 300, step1(False, 2, False), start="regen", use_phi=False, obs=None)
case("step1_then_k_featurize_small_unforced_batch", "cramped_room", 200, step1(True, 1, True), obs="features")
# ---- fused, k_train_step_obs: its smallest batch is N_OBS envs
case("obs_one_pot_u8_16_waves", "cramped_room", N_OBS + 232, obs_k(1, "u8", 16), **BIG)
case("obs_two_pots_u8_8_waves_one_env_in_the_last_workgroup", "coordination_ring", N_OBS + 1, obs_k(2, "u8", 8), **BIG)
case("obs_two_pots_f32_8_waves", "coordination_ring", N_OBS + 65, obs_k(2, "f32", 8), obs="f32", **BIG)
case("obs_two_pots_u8_16_waves", "cramped_room_two_pots", N_OBS, obs_k(2, "u8", 16), **BIG)
case("obs_one_pot_u8_8_waves_no_potential", "scenario2_s", N_OBS + 65, obs_k(1, "u8", 8), use_phi=False, **BIG)
case("obs_one_pot_f32_8_waves", "cramped_room", N_OBS + 1, obs_k(1, "f32", 8), obs="f32", **BIG)
# ---- not fused: k_sample_actions, then the step's own path
case("unfused_event_sink", "cramped_room", 200, unfused(TC.step_k(True, True)), events=1, claims=("all_actions",))
case("unfused_65_cells", "marshmallow_experiment", 300, unfused(TC.step_k(True, False)), obs="f32")
case("unfused_seven_pots_sequence", "seven_pots", 200, unfused("sequence: oc_step"))
# ---- argmax mode, fused and not
case("greedy_feat_ragged_last_workgroup", "cramped_room", RAGGED, feat_k(1), greedy=True, **FEAT)
case("greedy_unfused_event_sink", "cramped_room", 200, unfused(TC.step_k(True, True)), events=1, greedy=True)
CASES = tuple(CASES)
assert len({c.id for c in CASES}) == len(CASES)


def by_id(id):
    return next(c for c in CASES if c.id == id)


def far_case():
    """A fused case at the far corner of the counter space (tests/far_cases.py): a seed with both halves set, an env offset whose low
    word wraps inside the batch, and a sample counter that starts at 2^32 - 3 (t_lo wraps and t_hi goes 0 -> 1 inside the run)."""
    import far_cases as F

    c = by_id("feat_ragged_last_workgroup")
    return c._replace(id=c.id + "@far", seed=F.FAR_SEED, env_offset=F.far_env_offset(c.n_envs), step0=2**32 - 3)


def instance_of(c):
    """The SAMPLE instance a fused case is there for; None for the others."""
    return None if c.expect.startswith("k_sample_actions") else c.expect


def plan_of_case(c):
    """oc_multi_agent_step_sample_plan's answer for the call VecOvercookedMultiAgent.step_sampled makes of the case."""
    from overcooked_ai_amd import _lib, dispatch

    return dispatch.multi_agent_sample_plan(
        table_of(c.table), c.n_envs, horizon=c.horizon, obs_dtype=_lib.OBS_F32 if c.obs == "f32" else _lib.OBS_U8,
        with_obs=c.obs in ("u8", "f32"), with_features=c.obs == "features", num_pots=c.num_pots,
        options=_lib.OPT_ONE_KERNEL if c.one_kernel else 0, use_phi=c.use_phi, event_sink=c.events, start=start_spec_of(c))


def env_kwargs(c):
    """Keyword arguments of the VecOvercookedMultiAgent the case steps (layouts, n_envs, device and obs_dtype aside)."""
    kw = dict(horizon=c.horizon, use_phi=c.use_phi, gamma=GAMMA, seed=c.seed, env_offset=c.env_offset, layout_id=layout_ids(c),
              track_events=bool(c.events), obs={"u8": "ppo", "f32": "ppo", None: "bc", "features": "features"}[c.obs],
              num_pots=c.num_pots, counter_goals=c.counter_goals, one_kernel=c.one_kernel, reward_shaping_factor=c.factor)
    if c.start != "standard":
        kw.update(DRAWN)
    if c.start == "regen":
        kw["regen_layout"] = True
    return kw


def nan_rows(c, t):
    """[(env, player, action index)]: the logits that are NaN at step t — N_BAD rows no two steps share, spread over the batch; none on
    batches of fewer than 127 envs."""
    if c.n_envs < 127:
        return []
    stride = (c.n_envs - 2) // (N_BAD * c.steps)
    assert stride >= 1
    return [((N_BAD * t + k) * stride, (t + k) & 1, (t + 2 * k) % 6) for k in range(N_BAD)]


def logits_of(c, t):
    """float32 [n_envs, 2, 6], C-contiguous: the policy's output at step t of the case."""
    rng = np.random.default_rng([c.seed & 0xFFFFFFFF, t, 0x10617])
    l = (rng.standard_normal((c.n_envs, 2, 6)) * 3.0).astype(np.float32)
    masked = rng.random((c.n_envs, 2, 6)) < 0.1
    masked[..., 0] &= ~masked.all(axis=-1)  # never a whole row
    l[masked] = -np.inf
    for e, p, i in nan_rows(c, t):
        l[e, p, i] = np.nan
    return np.ascontiguousarray(l)


def uniforms_of(c, t, n_envs=None, e0=0):
    return uniforms(c.seed, c.env_offset + e0, c.step0 + t, c.n_envs if n_envs is None else n_envs)


def oracle_of(c):
    return TC.oracle_of(c)


def features_of(c, ref):
    """float32 [n_envs, 2, total]: oracle.featurize of the states the reference's next step starts from."""
    return np.asarray(ref.O.featurize(ref.orc, ref.state, counter_goals=c.counter_goals, num_pots=c.num_pots, layout_id=ref.layout_id),
                      dtype=np.float32)


def total_of(num_pots):
    return 2 * (num_pots * 10 + 26) + 4
