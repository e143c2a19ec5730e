"""The cases on which oc_bc_epoch_fused (csrc/bc_fused.hpp) is held to oc_bc_update bit for bit, and what numpy alone says of them: the
index, the actions, the minibatches and the rows each minibatch leaves out.  numpy only; imported like helpers.py.

A case is an epoch: R feature rows with an action each, an index of n entries cut into minibatches of M rows, a network shape,
class weights ("off", "on", or "zero": on with one zero weight), clipping or none.  The index of every case repeats entries and holds
entries out of range on both sides (negative, and >= R); the actions hold 255 (the sampler's invalid row) and 6 (above 5).
Specials:
  middle_out    the middle minibatch names no sample at all: it is skipped, clock[3] counts it
  nan_left_out  rows 32..63 of the one 64-row minibatch are left out (their actions are 255) and their feature rows hold NaN: the
                second wavefront's tile has 32 zero upstream rows and its backward pass is skipped, so no NaN reaches a gradient
  nan_kept      a kept row of the middle minibatch has a NaN feature: the norm is not finite and the minibatch is skipped
  chain         one more minibatch (of one row) than a launch holds: two launches"""
import collections
import functools
import re

import numpy as np

FILL = -7.0     # what stats and info start as, and their guard rows
MAX_ROWS = 128  # the largest minibatch the fused kernel serves
SERVED_IN_DIMS = (56, 76, 96)
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
CLIP = 0.05     # a max_grad_norm below the norms of these cases' first steps (about 0.1 to 1): the clip factor is below 1

Case = collections.namedtuple("Case", "id in_dim h1 h2 n M weights clip special seed")


@functools.lru_cache(maxsize=None)
def per_launch():
    """The minibatches of one launch, at most, read from oc_bc_epoch_fused_plan's words (no device needed)."""
    from overcooked_ai_amd.bc import plan_bc_epoch_fused

    return int(re.search(r"at most (\d+) minibatches per launch", plan_bc_epoch_fused(1, 1)).group(1))


def _cases():
    out = []

    def add(in_dim, h1, h2, n, M, weights, clip, special=""):
        name = "%d_%d_%d-n%d-M%d-w_%s-%s%s" % (in_dim, h1, h2, n, M, weights, "clip" if clip else "noclip", "-" + special if special else "")
        out.append(Case(name, in_dim, h1, h2, n, M, weights, clip, special, 9100 + len(out)))

    modes = ("off", "on", "zero")
    for i, M in enumerate((1, 31, 32, 33, 64, 96, 97, 128)):  # every count of tiles, a full and a ragged last one; K = 1
        add(96, 64, 64, M, M, modes[i % 3], bool(i & 1))
    for i, in_dim in enumerate(SERVED_IN_DIMS):  # K = 3 with a shorter last minibatch (64, 64, 22), every instance, both pairs of widths
        add(in_dim, 64, 64, 150, 64, modes[i % 3], bool(i & 1))
        add(in_dim, 40, 24, 150, 64, modes[(i + 1) % 3], not (i & 1))
    for weights in modes:  # every weight mode with and without clipping at the reference's size
        for clip in (False, True):
            add(96, 64, 64, 130, 64, weights, clip)
    add(56, 1, 1, 70, 33, "on", True)
    add(96, 64, 64, 96, 32, "on", False, "middle_out")
    add(96, 64, 64, 64, 64, "off", False, "nan_left_out")
    add(96, 64, 64, 192, 64, "on", True, "nan_kept")
    add(76, 40, 24, per_launch() + 1, 1, "off", False, "chain")
    return out


def minibatches(c):
    """[(lo, hi)] of the index entries of every minibatch"""
    return [(lo, min(lo + c.M, c.n)) for lo in range(0, c.n, c.M)]


@functools.lru_cache(maxsize=None)
def arrays_of(c):
    """features f32 [R, in_dim], actions u8 [R], index i32 [n], class_weights f32 [6] or None, the eight initial weight arrays
    (tests/policy_cases.py's), read-only"""
    import policy_cases as PC

    rng = np.random.default_rng(c.seed)
    R = max(2 * c.n, 300)
    feats = rng.standard_normal((R, c.in_dim)).astype(np.float32)
    actions = rng.choice(6, size=R, p=(0.05, 0.05, 0.08, 0.08, 0.64, 0.10)).astype(np.uint8)
    actions[rng.random(R) < 0.03] = 255
    actions[rng.random(R) < 0.02] = 6
    index = rng.integers(0, R, c.n).astype(np.int32)
    if c.n >= 8:
        index[rng.choice(c.n, c.n // 8, replace=False)] = index[0]                          # repeats
        out = rng.choice(c.n, max(c.n // 16, 4), replace=False)
        index[out] = np.resize(np.array([-1, R, -77, R + 5, -2 ** 31, 2 ** 31 - 1], np.int64), len(out)).astype(np.int32)
        named = index[(index >= 0) & (index < R)]
        actions[named[1]], actions[named[2]] = 255, 6  # (an invalid action and one above 5 that the index names, whatever the draw)
    if c.special == "middle_out":
        index[c.M:2 * c.M] = np.resize(np.array([-1, R, -9, R + 1]), c.M)
    if c.special == "nan_left_out":
        index = np.arange(c.n, dtype=np.int32)  # (no repeats: rows 32..63 are named by the second tile alone)
        actions[:32] = np.minimum(actions[:32], 5)
        actions[32:64] = 255
        feats[32:64, ::3] = np.nan
    if c.special == "nan_kept":
        row = int(index[c.M + 5]) if 0 <= index[c.M + 5] < R else 7
        index[c.M + 5] = row
        index[:c.M] = np.where(index[:c.M] == row, (row + 1) % R, index[:c.M])          # only the middle minibatch names the row
        index[2 * c.M:] = np.where(index[2 * c.M:] == row, (row + 1) % R, index[2 * c.M:])
        actions[row] = 2
        feats[row, 11] = np.nan
    cw = None
    if c.weights != "off":
        cw = rng.uniform(0.25, 4.0, 6).astype(np.float32)
        if c.weights == "zero":
            cw[4] = 0.0
    weights = PC.weights_of(PC.Case("fused", c.n, c.in_dim, c.h1, c.h2, "indexed", "dense", c.seed + 1))
    for x in (feats, actions, index) + tuple(weights) + ((cw,) if cw is not None else ()):
        x.setflags(write=False)
    return feats, actions, index, cw, tuple(weights)


def left_out(c):
    """bool [n]: the index entry names no sample, or its action is above 5"""
    feats, actions, index, _, _ = arrays_of(c)
    ix = index.astype(np.int64)
    inside = (ix >= 0) & (ix < len(actions))
    return ~inside | (actions[np.where(inside, ix, 0)] > 5)


def kept_counts(c):
    """the count of kept rows of every minibatch"""
    out = left_out(c)
    return [int((~out[lo:hi]).sum()) for lo, hi in minibatches(c)]


CASES = _cases()
