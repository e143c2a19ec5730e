"""What the GPU tests share and torch is needed for: the device fixture, output arrays with guard rows, the packed event counters,
and the env and oracle constructors of the parity tests.  Imported like helpers.py; tests/case_support.py holds what needs no torch."""
import numpy as np
import pytest
import torch

from case_support import new_oracle

GUARD = 3  # guard rows behind (and, where asked, before) an output array


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test run without a GPU")
    from overcooked_ai_amd import _lib

    _lib.load()  # fail loudly if the HIP extension is missing
    return torch.device("cuda:0")


def guarded(rows, row_shape, dtype, fill, device, before=0):
    """(rows [before, before + rows) of a new array of before + rows + GUARD rows, all of it `fill`, a value no result holds; its
    guard slices: the rows behind the output and, with before > 0, those before it)."""
    whole = torch.full((before + rows + GUARD,) + tuple(row_shape), fill, dtype=dtype, device=device)
    return whole[before:before + rows], (whole[before + rows:],) + ((whole[:before],) if before else ())


def guards_untouched(case, what, guards, fill):
    """Every guard row of the array `what` still holds `fill`."""
    if not all(bool((g == fill).all()) for g in guards):
        pytest.fail("%s: guard rows of the %s written" % (getattr(case, "id", case), what))


def packed_counters(t):
    """[n_envs, 25] int32, player 0 in the low half-word -> [n_envs, 25, 2]"""
    c = t.cpu().numpy().astype(np.int64)
    return np.stack([c & 0xFFFF, (c >> 16) & 0xFFFF], -1)


def make_env(layouts, n, gpu, **kw):
    from overcooked_ai_amd.vec_env import VecOvercookedEnv

    return VecOvercookedEnv(layouts, n, device=gpu, **kw)


def oracle_for(specs):
    return new_oracle(specs if isinstance(specs, (list, tuple)) else [specs])
