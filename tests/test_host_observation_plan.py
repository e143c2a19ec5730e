"""oc_observation_plan without a GPU: the plans oc_encode_lossless and oc_rollout_encode make of a call before they launch (csrc/
observation_plan.hpp), put into words.  The expected numbers are worked out here from the rules, not read off the library.

The rules, for a W x H grid (cells = W * H, n_obj = ceil(cells / 16) object planes, n_planes = 1 + n_obj) and T = u8 / f32:
  env_bytes = 2 * cells * 26 * sizeof(T);  unit = the fewest envs whose bytes are a multiple of 16 (1, 2 or 4)
  k_encode           epb = 40960 // (env_bytes + 16 * n_planes), rounded down to a multiple of 4 when >= 4, at most 32
                     LDS = 16 * epb * n_planes + epb * env_bytes rounded up to 16;  grid = ceil(n_envs / epb)
  k_encode_uniform   (one layout, u8) upg = min(19 * env_bytes, 40960) // (unit * env_bytes), unit * upg <= 32
                     LDS = unit * env_bytes * (1 + upg) + 16 * unit * upg * n_planes
                     grid = min(256 CUs * min(8, 153600 // (LDS + 512)), ceil(n_envs / (unit * upg)))
  k_rollout_encode   (one layout, 1..2 pots, n_obj <= 3; n_envs >= 256 * 192 and n_steps >= 2, or OC_OPT_ONE_KERNEL)
                     fixed = 8192 * n_obj + unit * env_bytes + 4096 + 7424;  images of 8 wavefronts hold
                     gmax = (budget - fixed) // (8 * env_bytes) envs; fewer than 4 (u8) / 8 (f32): 4 wavefronts, twice that;
                     span = 32 (8 wavefronts) / 64 envs in parts = ceil(span / gmax) sub-groups of G = ceil(span / parts), rounded up
                     to unit, or gmax rounded down to unit where that is more than gmax;  LDS = fixed + NW * G * env_bytes
The LDS budget of k_rollout_encode is asked of the runtime (160 KiB less the instance's static LDS of 5-6 KiB and 64 bytes:
about 157 900 .. 158 600 bytes) and assumed to be 147 456 bytes where there is no device; the text says which.  Every case below has
the same answer for any budget from 147 456 to 160 000 bytes unless it says otherwise."""
import ctypes

import pytest

from case_support import P, observation_plan as plan, synthetic_batch as batch
from overcooked_ai_amd import _lib

ONE_KERNEL, AUTO_RESET = _lib.OPT_ONE_KERNEL, _lib.OPT_AUTO_RESET
U8, F32 = _lib.OBS_U8, _lib.OBS_F32


ENCODE = [
    # 5x4 u8, one layout: env_bytes 1040, unit 1, upg = 19760 // 1040 = 19, LDS = 1040 * 20 + 16 * 19 * 3 = 21712,
    # 153600 // 22224 = 6 groups per CU -> 1536 <= ceil(65536 / 19) = 3450
    (batch(5, 4, 65536), U8, "k_encode_uniform<T=u8> unit=1, upg=19, grid=1536, 21712 B LDS"),
    # 9x5 u8: env_bytes 2340 = 4 mod 16 -> unit 4; upg = 40960 // 9360 = 4; LDS = 9360 * 5 + 16 * 16 * 4 = 47824; 153600 // 48336 = 3
    (batch(9, 5, 65536, max_pots=2), U8, "k_encode_uniform<T=u8> unit=4, upg=4, grid=768, 47824 B LDS"),
    # 5x5 u8 (odd cells): env_bytes 1300 -> unit 4; upg = 24700 // 5200 = 4; LDS = 5200 * 5 + 16 * 16 * 3 = 26768; 17 groups of 16 envs
    (batch(5, 5, 257), U8, "k_encode_uniform<T=u8> unit=4, upg=4, grid=17, 26768 B LDS"),
    # 9x5 u8, five layouts: epb = 40960 // (2340 + 64) = 17 -> 16; LDS = 16 * 16 * 4 + 37440 = 38464; ceil(1000 / 16) = 63
    (batch(9, 5, 1000, n_layouts=5, max_pots=2), U8, "k_encode<T=u8, LAY_LDS=true> epb=16, grid=63, 38464 B LDS"),
    # 5x5 u8, two layouts: epb = 40960 // 1348 = 30 -> 28 (28 * 1300 = 36400 is a multiple of 16); LDS = 1344 + 36400; ceil(257 / 28) = 10
    (batch(5, 5, 257, n_layouts=2), U8, "k_encode<T=u8, LAY_LDS=true> epb=28, grid=10, 37744 B LDS"),
    # ... a table of 33 layouts is read through L2
    (batch(9, 5, 257, n_layouts=33, max_pots=2), U8, "k_encode<T=u8, LAY_LDS=false> epb=16, grid=17, 38464 B LDS"),
    # 5x4 f32 (one layout: f32 never takes the template kernel): epb = 40960 // (4160 + 48) = 9 -> 8; LDS = 384 + 33280
    (batch(5, 4, 63), F32, "k_encode<T=f32, LAY_LDS=true> epb=8, grid=8, 33664 B LDS"),
    # 9x5 f32, 40 layouts: epb = 40960 // (9360 + 64) = 4; LDS = 256 + 37440
    (batch(9, 5, 1, n_layouts=40, max_pots=2), F32, "k_encode<T=f32, LAY_LDS=false> epb=4, grid=1, 37696 B LDS"),
]


@pytest.mark.parametrize("b,dtype,want", ENCODE, ids=[w.split(">")[0] + ">" + "/%dx%d" % (b.width, b.height) for b, _, w in ENCODE])
def test_encode_plan(b, dtype, want):
    assert plan(b, dtype) == (0, want)
    # horizon, options, the arrays and the start spec are not part of an encode call: not read
    assert plan(b, dtype, 0, 0xFFFF, 1, 0, _lib.OcStartSpec(0, 0, 0, 0, 7.0, 0, 0), horizon=0) == (0, want)


def rollout_text(fast, t, nw, unit, g, lds):
    return "k_rollout_encode<MAXP=2, FAST=%d, T=%s, NW=%d> unit=%d, G=%d, %d B LDS, budget " % (fast, t, nw, unit, g, lds)


ROLLOUT = [
    # 5x4 u8: fixed = 16384 + 1040 + 11520 = 28944; gmax = 118512 // 8320 = 14 (15 from 158 000 bytes: the same three parts) -> 8
    # wavefronts, 32 envs in 3 parts of 11; LDS = 28944 + 88 * 1040
    (batch(5, 4, 65536), U8, 40, AUTO_RESET, rollout_text(3, "u8", 8, 1, 11, 120464)),
    # 9x5 u8: unit 4, fixed = 24576 + 9360 + 11520 = 45456; gmax = 102000 // 18720 = 5 (6 from 158 000) -> 8 wavefronts; 7 (6) parts of
    # 5 (6) envs, rounded up to the unit 8 > gmax -> 4; LDS = 45456 + 32 * 2340
    (batch(9, 5, 49152, max_pots=2), U8, 2, 0, rollout_text(3, "u8", 8, 4, 4, 120336)),
    # the same table without the two-players hint: FAST=0
    (batch(9, 5, 260, max_pots=2, flags=0), U8, 1, ONE_KERNEL, rollout_text(0, "u8", 8, 4, 4, 120336)),
    # 3x3 f32: env_bytes 1872, fixed = 8192 + 1872 + 11520 = 21584; gmax = 125872 // 14976 = 8 (9 from 158 000: four parts either
    # way) -> 8 wavefronts, 4 parts of 8; LDS = 21584 + 64 * 1872
    (batch(3, 3, 260), F32, 12, ONE_KERNEL | AUTO_RESET, rollout_text(3, "f32", 8, 1, 8, 141392)),
    (batch(3, 3, 260, flags=0), F32, 12, ONE_KERNEL, rollout_text(0, "f32", 8, 1, 8, 141392)),
    # 4x3 f32: env_bytes 2496, fixed = 8192 + 2496 + 11520 = 22208; gmax = 125248 // 19968 = 6 < 8 -> 4 wavefronts: gmax = 12 (13 from
    # 158 000), 64 envs in 6 (5) parts of 11 (13): the instance holds for any budget, G does not
    (batch(4, 3, 65536), F32, 2, 0, "k_rollout_encode<MAXP=2, FAST=3, T=f32, NW=4> unit=1, G="),
    (batch(4, 3, 65536, flags=0), F32, 2, 0, "k_rollout_encode<MAXP=2, FAST=0, T=f32, NW=4> unit=1, G="),
]


@pytest.mark.parametrize("b,dtype,n_steps,options,want", ROLLOUT, ids=[w.split(">")[0] + ">" for *_, w in ROLLOUT])
def test_rollout_encode_plan(b, dtype, n_steps, options, want):
    rc, text = plan(b, dtype, n_steps, options)
    assert rc == 0 and text.startswith(want), text
    budget, how = text.rsplit("budget ", 1)[1].split(" B ")
    assert how in ("(queried)", "(fallback)") and (int(budget) == 147456 if how == "(fallback)" else 147456 < int(budget) < 160000), text
    assert plan(b, dtype, n_steps, options, actions=1) == (0, text)  # (whose actions: not the single kernel's concern)


def test_no_budget_from_144_kib_up_reaches_the_four_wavefront_u8_instances():
    """k_rollout_encode<.., T=u8, NW=4> needs eight images of fewer than 4 envs (or of less than a unit); the largest u8 grids the
    kernel takes — 48 cells: gmax = (147456 - 38592) // (8 * 2496) = 5; 45 cells: 5, see above — still hold 5.  Those two instances
    are there for smaller budgets and for the tuning knob OC_ROLLOUT_ENCODE_WAVES; and no grid fails to fit four images (9x5 f32:
    (147456 - 45456) // (4 * 9360) = 2 envs), so "does not fit: step by step" needs a smaller budget too."""
    for w in range(3, 17):
        for h in range(3, 17):
            if w * h <= 48:
                for dtype in (U8, F32):
                    rc, text = plan(batch(w, h, 260), dtype, 2, ONE_KERNEL)
                    assert rc == 0 and text.startswith("k_rollout_encode<") and (dtype == F32 or "NW=8>" in text), (w, h, text)


def test_which_calls_take_the_single_kernel():
    """The rule before the shape: every CU a workgroup of 192 envs (256 * 192 = 49 152 envs) and at least two steps, or
    OC_OPT_ONE_KERNEL; one layout, one or two pots, at most 48 cells.  Everything else is the one-step entry points step by step, and
    the text goes on with the encode instance of each step."""
    uniform = "k_encode_uniform<T=u8> unit=1, upg=19, grid="
    assert plan(batch(5, 4, 49152), U8, 2)[1].startswith("k_rollout_encode<MAXP=2, FAST=3, T=u8, NW=8>")
    assert plan(batch(5, 4, 49151), U8, 2)[1].startswith("step by step: oc_rollout_random + " + uniform)
    assert plan(batch(5, 4, 49152), U8, 1)[1].startswith("step by step: oc_rollout_random + " + uniform)
    assert plan(batch(5, 4, 49152), U8, 1, actions=1)[1].startswith("step by step: oc_step + " + uniform)
    assert plan(batch(5, 4, 1), U8, 1, ONE_KERNEL)[1].startswith("k_rollout_encode<MAXP=2, FAST=3, T=u8, NW=8>")
    for other in (batch(5, 4, 65536, n_layouts=2), batch(5, 4, 65536, max_pots=0), batch(5, 4, 65536, max_pots=3), batch(7, 7, 65536)):
        rc, text = plan(other, U8, 40, ONE_KERNEL | AUTO_RESET)
        assert rc == 0 and text.startswith("step by step: oc_rollout_random + k_encode"), text
    # seven pots on 7x4 (env_bytes 1456, unit 1, upg 19: LDS = 1456 * 20 + 912 = 30032; ceil(5004 / 19) = 264 groups), f32 on 9x5 x 5 layouts
    assert plan(batch(7, 4, 5004, max_pots=7), U8, 40, ONE_KERNEL | AUTO_RESET) == \
        (0, "step by step: oc_rollout_random + k_encode_uniform<T=u8> unit=1, upg=19, grid=264, 30032 B LDS")
    assert plan(batch(9, 5, 3000, n_layouts=5, max_pots=2), F32, 30, ONE_KERNEL, actions=1) == \
        (0, "step by step: oc_step + k_encode<T=f32, LAY_LDS=true> epb=4, grid=750, 37696 B LDS")


def test_nothing_to_launch():
    assert plan(batch(5, 4, 0)) == (0, "nothing to launch (no envs)")
    assert plan(batch(5, 4, 0), F32, 40, ONE_KERNEL) == (0, "nothing to launch (no envs)")
    # (n_steps == 0 is the question about oc_encode_lossless; oc_rollout_encode's own empty call is seen through the entry point)
    L = _lib.load()
    b = batch(5, 4, 100)
    assert L.oc_rollout_encode(ctypes.byref(b), P, None, None, None, None, P, U8, 0, 400, 1, 0, 0, 0, 0, None, None) == 0


def test_refusals_in_the_order_of_the_checks():
    """Each refusal comes back as the entry point's code and message; with several faults at once the first check in the entry
    point's order answers."""
    L = _lib.load()
    ok = batch(5, 4, 100)
    bad_thresh = _lib.OcStartSpec(3, 0, 1, 0, 2.0, 0, 0)
    bad_regen = _lib.OcStartSpec(3, 0, 1, 0, 0.5, 0, 2)  # (a layout range beyond the table of one)
    out = ctypes.create_string_buffer(320)
    assert L.oc_observation_plan(ctypes.byref(ok), U8, 400, 0, 0, 0, 1, None, None, 0) == -1
    assert L.oc_last_error().decode() == "oc_observation_plan: no output buffer"
    assert L.oc_observation_plan(ctypes.byref(ok), U8, 400, 0, 2, 0, 1, None, out, 0) == -1
    assert L.oc_last_error().decode() == "oc_observation_plan: no output buffer"
    batches = [(None, "batch is NULL"),
               (_lib.OcBatch(d_layouts=None, n_envs=100, n_layouts=1, width=5, height=4), "batch.d_layouts is NULL"),
               (batch(5, 4, -1), "batch.n_envs < 0"),
               (batch(5, 4, 100, n_layouts=0), "batch.n_layouts out of range (1..65536)"),
               (_lib.OcBatch(d_layouts=P, d_layout_id=None, n_envs=100, n_layouts=2, width=5, height=4), "d_layout_id required when n_layouts > 1"),
               (batch(2, 9, 100), "grid shape out of range (3x3 .. 128 cells)"),
               (batch(43, 3, 100), "grid shape out of range (3x3 .. 128 cells)")]
    for n_steps in (0, 2):
        for b, why in batches:  # (with every later fault as well)
            assert plan(b, 7, n_steps, 0x8, 1, 0, bad_thresh, horizon=0) == (-1, why), (n_steps, why)
    # oc_encode_lossless: the batch, (the pointers), the type, (the alignment)
    assert plan(ok, 2) == (-1, "oc_encode_lossless: bad obs_dtype")
    assert plan(ok, -1) == (-1, "oc_encode_lossless: bad obs_dtype")
    # oc_rollout_encode: the batch, the start spec, (the pointers), the type, (the alignment), the horizon, the steps, the options,
    # the arrays caller actions need
    start_rule = "oc_rollout_encode: start.rnd_obj_prob_thresh must be in [0, 1] and its regen range within the table"
    ladder = [(dict(start=bad_thresh), start_rule), (dict(start=bad_regen), start_rule),
              (dict(dtype=2), "oc_rollout_encode: bad obs_dtype"),
              (dict(horizon=0), "oc_rollout_encode: horizon must be in 1..65535"),
              (dict(n_steps=-1), "oc_rollout_encode: n_steps must be in 0..2^30"),
              (dict(options=_lib.OPT_FLAGS_TILED8), "oc_rollout_encode: options other than OC_OPT_AUTO_RESET / OC_OPT_ONE_KERNEL"),
              (dict(actions=1, outputs=0), "oc_rollout_encode: caller actions need the rewards and flags arrays")]
    for k, (_, why) in enumerate(ladder):
        kw = dict(n_steps=2, options=0)
        for later, _ in reversed(ladder[k:]):  # this fault and every later one: this one answers
            kw.update(later)
        assert plan(ok, **kw) == (-1, why), why
    assert plan(ok, U8, (1 << 30) + 1)[1] == "oc_rollout_encode: n_steps must be in 0..2^30"
    assert plan(ok, U8, 2, horizon=65536)[1] == "oc_rollout_encode: horizon must be in 1..65535"
    assert plan(ok, U8, 2, AUTO_RESET, start=_lib.OcStartSpec(3, 64, 1, 1, 0.5, 0, 0))[0] == 0  # (the call described carries the spec's env offset)
    # the checks a plan's arguments cannot fail, at the entry points themselves (no launch: every one is refused first)
    br = ctypes.byref(ok)
    assert L.oc_encode_lossless(br, None, P, U8, 400, None) == -1 and L.oc_last_error().decode() == "oc_encode_lossless: NULL pointer"
    assert L.oc_encode_lossless(br, P, None, U8, 400, None) == -1 and L.oc_last_error().decode() == "oc_encode_lossless: NULL pointer"
    assert L.oc_encode_lossless(br, P, P + 8, U8, 400, None) == -1 and L.oc_last_error().decode() == "oc_encode_lossless: d_obs must be 16-byte aligned"
    assert L.oc_encode_lossless(br, P, P + 8, 5, 400, None) == -1 and L.oc_last_error().decode() == "oc_encode_lossless: bad obs_dtype"
    re = lambda d_state, d_obs, stride, offset, start: L.oc_rollout_encode(  # noqa: E731
        br, d_state, None, None, None, None, d_obs, U8, stride, 400, 1, 0, offset, 0, 3, start, None)
    assert re(None, P, 0, 0, None) == -1 and L.oc_last_error().decode() == "oc_rollout_encode: NULL state / observation pointer"
    assert re(P, None, 0, 0, None) == -1 and L.oc_last_error().decode() == "oc_rollout_encode: NULL state / observation pointer"
    for d_obs, stride in ((P + 4, 0), (P, 24), (P, -16)):
        assert re(P, d_obs, stride, 0, None) == -1
        assert L.oc_last_error().decode() == "oc_rollout_encode: d_obs and obs_step_stride must be multiples of 16 bytes"
    assert re(P, P, 0, 64, ctypes.byref(_lib.OcStartSpec(3, 0, 1, 1, 0.5, 0, 0))) == -1
    assert L.oc_last_error().decode() == "oc_rollout_encode: start.env_offset differs from env_offset"
    assert L.oc_step_encode(br, P, P, P, P, None, P + 8, U8, 400, 1, None, None) == -1
    assert L.oc_last_error().decode() == "oc_step_encode: d_obs must be 16-byte aligned"
    assert L.oc_step_encode(br, P, P, P, P, None, P, 3, 400, 1, None, None) == -1 and L.oc_last_error().decode() == "oc_step_encode: bad obs_dtype"
    assert L.oc_step_encode(br, P, P, P, P, None, P, U8, 400, 1, ctypes.byref(bad_thresh), None) == -1
    assert L.oc_last_error().decode() == start_rule.replace("oc_rollout_encode", "oc_step_encode")


def test_the_plan_of_a_layout_table_with_stand_in_pointers():
    """dispatch.observation_plan: the hints come from the table (oc_batch_hints), the pointers are stand-ins."""
    from overcooked_ai_amd import dispatch
    from overcooked_ai_amd.layouts import LayoutTable, spec_from_name

    cramped, asym = LayoutTable([spec_from_name("cramped_room")]), LayoutTable([spec_from_name("asymmetric_advantages")])
    assert dispatch.observation_plan(cramped, 65536) == ENCODE[0][2]
    assert dispatch.observation_plan(asym, 65536) == ENCODE[1][2]
    assert dispatch.observation_plan(cramped, 65536, 40).startswith(ROLLOUT[0][4])
    assert dispatch.observation_plan(asym, 260, 12, options=ONE_KERNEL).startswith(ROLLOUT[1][4])
    assert dispatch.observation_plan(asym, 260, 12, _lib.OBS_F32) == "step by step: oc_rollout_random + k_encode<T=f32, LAY_LDS=true> epb=4, grid=65, 37696 B LDS"
    mix = LayoutTable([spec_from_name(nm) for nm in ("cramped_room", "asymmetric_advantages")], pad_to=(9, 5))
    assert dispatch.observation_plan(mix, 1000, 3, with_actions=True, options=ONE_KERNEL) == \
        "step by step: oc_step + k_encode<T=u8, LAY_LDS=true> epb=16, grid=63, 38464 B LDS"
    with pytest.raises(_lib.OcAmdError, match="oc_rollout_encode: horizon must be in 1..65535"):
        dispatch.observation_plan(cramped, 100, 2, horizon=0)
