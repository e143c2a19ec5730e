"""Which rollout kernel instance serves which batch, which path and kernel instance a training step takes, and which kernel
instance writes an observation, and which kernel instance steps a batch with the caller's actions: the host side of
oc_rollout_plan, oc_multi_agent_plan, oc_observation_plan and oc_step_plan (include/oc_amd.h, ABI 6).

The answers are the plans oc_rollout_random, oc_multi_agent_step, oc_encode_lossless, oc_rollout_encode, oc_step, oc_step_many
and oc_step_server_open make of a call before
they launch anything, put into words (the planners hold no launch and no device pointer), so this works on a host without a GPU.  `table()` is what tools/gen_dispatch_table.py writes to docs/DISPATCH.md and
what tests/test_dispatch_table.py compares that file with."""
import ctypes

import numpy as np

from . import _lib, layouts


def batch_for(table, n_envs):
    """OcBatch of `n_envs` envs over a LayoutTable with the kernel-variant hints filled in; stand-in device pointers."""
    L = _lib.load()
    b = _lib.OcBatch(d_layouts=4096, d_layout_id=4096 if len(table) > 1 else None, n_envs=int(n_envs), n_layouts=len(table),
                     width=table.width, height=table.height)
    rec = np.ascontiguousarray(table.records)
    _lib.check(L.oc_batch_hints(rec.ctypes.data, len(table), ctypes.byref(b)), "oc_batch_hints")
    return b


def rollout_plan(table, n_envs, n_steps=4000, t0=0, horizon=400, options=_lib.OPT_AUTO_RESET, with_outputs=True, event_sink=0,
                 start=None):
    """The kernel instance `oc_rollout_random` launches for this table and launch shape (text), or the library's refusal
    (OcAmdError) for shapes it does not serve."""
    L = _lib.load()
    b = batch_for(table, n_envs)
    out = ctypes.create_string_buffer(320)
    rc = L.oc_rollout_plan(ctypes.byref(b), int(horizon), int(options), int(t0), int(n_steps), int(bool(with_outputs)),
                           int(event_sink), ctypes.byref(start) if start is not None else None, out, len(out))
    _lib.check(rc, "oc_rollout_plan")
    return out.value.decode()


def multi_agent_plan(table, n_envs, horizon=400, obs_dtype=_lib.OBS_F32, with_obs=True, use_phi=True, event_sink=0, start=None):
    """The path and kernel instance `oc_multi_agent_step` runs for this table, batch size and set of arrays (text; up to and
    including '>' the instance's name), or the library's refusal (OcAmdError).  obs_dtype: _lib.OBS_U8 / OBS_F32; event_sink: 0 or
    1 (per-episode counters); start: None or the OcStartSpec the call would carry."""
    L = _lib.load()
    b = batch_for(table, n_envs)
    out = ctypes.create_string_buffer(320)
    rc = L.oc_multi_agent_plan(ctypes.byref(b), int(horizon), int(bool(with_obs)), int(obs_dtype), int(bool(use_phi)), int(event_sink),
                               ctypes.byref(start) if start is not None else None, out, len(out))
    _lib.check(rc, "oc_multi_agent_plan")
    return out.value.decode()


def multi_agent_featurize_plan(table, n_envs, horizon=400, obs_dtype=_lib.OBS_F32, with_obs=False, with_features=True, num_pots=2,
                               options=0, use_phi=True, event_sink=0, start=None):
    """What `oc_multi_agent_step_featurize` runs for this table, batch size and set of arrays (text; up to and including '>' the
    instance's name): "k_train_step_feat<MAXP=..> ..." for the one-kernel path, else oc_multi_agent_plan's text followed by
    " + k_featurize<LAY_LDS=..> ..."; with_features=False: oc_multi_agent_plan's answer.  options: 0 or _lib.OPT_ONE_KERNEL; the
    other arguments as for multi_agent_plan.  The library's refusal is an OcAmdError."""
    L = _lib.load()
    b = batch_for(table, n_envs)
    out = ctypes.create_string_buffer(320)
    rc = L.oc_multi_agent_step_featurize_plan(ctypes.byref(b), int(horizon), int(bool(with_obs)), int(obs_dtype), int(bool(with_features)),
                                              int(num_pots), int(options), int(bool(use_phi)), int(event_sink),
                                              ctypes.byref(start) if start is not None else None, out, len(out))
    _lib.check(rc, "oc_multi_agent_step_featurize_plan")
    return out.value.decode()


def multi_agent_sample_plan(table, n_envs, horizon=400, obs_dtype=_lib.OBS_F32, with_obs=False, with_features=False, num_pots=2,
                            options=0, use_phi=True, event_sink=0, start=None):
    """What `oc_multi_agent_step_sample` runs for this table, batch size and set of arrays (text): the words of
    multi_agent_featurize_plan for the same call with ", SAMPLE=true" as the last parameter of the step kernel where that kernel draws
    the actions itself (k_train_step_obs, k_train_step_feat, k_train_step1), else behind "k_sample_actions + ".  The arguments as
    for multi_agent_featurize_plan.  The library's refusal is an OcAmdError."""
    L = _lib.load()
    b = batch_for(table, n_envs)
    out = ctypes.create_string_buffer(400)
    rc = L.oc_multi_agent_step_sample_plan(ctypes.byref(b), int(horizon), int(bool(with_obs)), int(obs_dtype), int(bool(with_features)),
                                           int(num_pots), int(options), int(bool(use_phi)), int(event_sink),
                                           ctypes.byref(start) if start is not None else None, out, len(out))
    _lib.check(rc, "oc_multi_agent_step_sample_plan")
    return out.value.decode()


def observation_plan(table, n_envs, n_steps=0, obs_dtype=_lib.OBS_U8, horizon=400, options=_lib.OPT_AUTO_RESET, with_actions=False,
                     with_outputs=True, start=None):
    """The kernel instance `oc_encode_lossless` (n_steps == 0) or `oc_rollout_encode` (n_steps >= 1) launches for this table and
    batch size, or "step by step: ..." with the one-step entry point and the encode instance of every step (text; up to and
    including '>' the instance's name), or the library's refusal (OcAmdError).  obs_dtype: _lib.OBS_U8 / OBS_F32; options:
    OPT_AUTO_RESET, OPT_ONE_KERNEL."""
    L = _lib.load()
    b = batch_for(table, n_envs)
    out = ctypes.create_string_buffer(320)
    rc = L.oc_observation_plan(ctypes.byref(b), int(obs_dtype), int(horizon), int(options), int(n_steps), int(bool(with_actions)),
                               int(bool(with_outputs)), ctypes.byref(start) if start is not None else None, out, len(out))
    _lib.check(rc, "oc_observation_plan")
    return out.value.decode()


STEP_ENTRIES = {"step": 0, "step_many": 1, "server": 2}  # oc_step_plan's `entry`


def step_plan(table, n_envs, entry="step", n_steps=1, horizon=400, options=_lib.OPT_AUTO_RESET, with_masks=False, with_counts=False,
              start=None, batch=None):
    """The kernel instance `oc_step` (entry "step"), `oc_step_many` ("step_many") or `oc_step_server_open` ("server") launches for
    this table and batch size (text; up to and including '>' the instance's name), "step by step: oc_step + ..." for oc_step_many
    with OPT_PREDICATE_INTERACT, or the library's refusal (OcAmdError).  with_masks / with_counts: per-step event masks / per-episode
    counters are asked for; batch: an OcBatch to plan for instead of batch_for(table, n_envs) (hints withheld, say)."""
    L = _lib.load()
    b = batch_for(table, n_envs) if batch is None else batch
    out = ctypes.create_string_buffer(320)
    rc = L.oc_step_plan(ctypes.byref(b), STEP_ENTRIES[entry], int(horizon), int(options), int(n_steps), int(bool(with_masks)),
                        int(bool(with_counts)), ctypes.byref(start) if start is not None else None, out, len(out))
    _lib.check(rc, "oc_step_plan")
    return out.value.decode()


# the launch shapes docs/DISPATCH.md lists per layout: (column title, kwargs)
SHAPES = (
    ("65 536 envs x 4 000 steps, tiled flags (bench.py's shape)", dict(n_envs=65536, options=_lib.OPT_AUTO_RESET | _lib.OPT_FLAGS_TILED8)),
    ("1 048 576 envs x 4 000 steps", dict(n_envs=1 << 20)),
    ("65 536 envs, per-episode event counters", dict(n_envs=65536, event_sink=1)),
    ("100 envs x 5 steps", dict(n_envs=100, n_steps=5)),
    ("65 536 envs x 4 000 steps, no output arrays", dict(n_envs=65536, with_outputs=False)),
)


def _short(text):
    """'k_rollout5<LAY_LDS=true, ...>[ one pot slot,] mover + ..., 130864 B LDS' -> instance name, pot slots, rounds, LDS bytes"""
    head = text.split(">")[0] + ">" if "<" in text else text
    lds = text.rsplit(",", 1)[-1].strip() if "B LDS" in text else ""
    rounds = [p.strip() for p in text.split(",") if "round(s)" in p]
    slots = " one pot slot" if "> one pot slot," in text else ""
    return head + slots + (" " + rounds[0] if rounds else "") + (" " + lds if lds else "")


def table(names=None):
    """Rows (layout, cells, pots, old_dynamics, [instance per SHAPES entry]) for every registry layout the library serves (two
    players), plus its old-dynamics form for the layouts the paper-reproduction runs use."""
    rows = []
    for name in (names or layouts.layout_names()):
        for old in (False, True):
            try:
                spec = layouts.spec_from_name(name, old_dynamics=True) if old else layouts.spec_from_name(name)
            except (AssertionError, ValueError):
                continue  # (old dynamics: three-item orders only, mdp.py:1121-1127)
            if old and name not in ("cramped_room", "asymmetric_advantages", "coordination_ring", "forced_coordination", "counter_circuit_o_1order"):
                continue
            if spec.num_players != 2:
                rows.append((name, spec.width * spec.height, len(spec.cells_of("P")), old, ["refused: %d players" % spec.num_players] * len(SHAPES)))
                continue
            tab = layouts.LayoutTable([spec])
            cols = []
            for _, kw in SHAPES:
                try:
                    cols.append(_short(rollout_plan(tab, **kw)))
                except _lib.OcAmdError as e:
                    cols.append("refused: " + str(e).split(": ", 2)[-1][:80])
            rows.append((name, tab.n_cells, tab.max_pots, old, cols))
    return rows


def render(rows):
    out = ["# Rollout dispatch per layout (generated: `python tools/gen_dispatch_table.py`; checked by tests/test_dispatch_table.py)", "",
           "What `oc_rollout_random` launches for a batch of ONE registry layout, as `oc_rollout_plan` (include/oc_amd.h) reports it — the",
           "plan the library makes of a call before it launches, in words.  `k_rollout5` = mover + interact wavefronts (csrc/step_duo5.hpp);",
           "`k_rollout4` = one wavefront per 64 envs (csrc/step_lut4.hpp: MODE 0 arithmetic movement, 1 joint move table, 2 floor mask).", "",
           "| layout | cells | pots | dynamics | " + " | ".join(t for t, _ in SHAPES) + " |", "|---|---|---|---|" + "---|" * len(SHAPES)]
    for name, cells, pots, old, cols in rows:
        out.append("| %s | %d | %d | %s | %s |" % (name, cells, pots, "old" if old else "new", " | ".join("`%s`" % c for c in cols)))
    return "\n".join(out) + "\n"
