"""CPU tests of the self-influence call: fia_self_influence is declared, exported and bound and
refuses a NULL context; the facade validates train_indices, K and full on the host -- ValueError
before any GPU call (the objects here have no GPU context); and the identities of the reference
the GPU tests compare against: for train row j = (a, b, y),

    group_reference(fo.query(..., a, b, ...), [j], ...)       (tests/test_group_cpu.py)

gives first_order (the sum of j's two influences in its own related list), group (the newton
value: the system without j's terms, solved again) and core["e"] at an occurrence of j.
"""
import ctypes

import numpy as np
import pytest

from influence import _lib
from influence.NCF import NCF
from influence.matrix_factorization import MF
from oracle import fia_oracle as fo

from test_abi import header_functions
from test_group_cpu import DAMP, WD, _bare, _problem, group_reference, w3g_of

# every test of this module is about fia_self_influence: without its binding nothing here runs
SELF_ARGTYPES = _lib.SIGNATURES["fia_self_influence"][1]


def self_reference(model, p, k, tu, ti, tr, j, wd, damping, W3g):
    """(first_order, newton, error, cond(H - H_j)) of train row j, from the group reference."""
    core = fo.query(model, p, k, tu, ti, tr, int(tu[j]), int(ti[j]), wd, damping)
    ref = group_reference(core, [j], wd, damping, W3g)
    occ = np.nonzero(core["rel"] == j)[0]
    assert occ.size == 2 and np.array_equal(occ, ref["occ"])
    assert core["e"][occ[0]] == core["e"][occ[1]]
    return ref["first_order"], ref["group"], float(core["e"][occ[0]]), ref["cond"], core, ref


def test_self_influence_declared_exported_bound(libfia_path):
    assert "fia_self_influence" in header_functions()
    assert hasattr(ctypes.CDLL(libfia_path), "fia_self_influence")
    assert "fia_self_influence" in _lib.SIGNATURES
    lib = _lib.load_library(libfia_path)
    assert len(SELF_ARGTYPES) == 11
    assert lib.fia_self_influence(None, 0, None, None, None, None, 0, None, None, None, None) == 1
    assert lib.fia_version() == 100
    assert hasattr(_lib.Context, "self_influence")


@pytest.mark.parametrize("cls", [MF, NCF])
def test_self_influence_host_validation(cls):
    m = _bare(cls)                                       # 20 train rows, no GPU context
    for bad in (np.array([1.0, 2.0]),                    # not integers
                [0.5],
                np.array([[1, 2]]),                      # not 1-d
                np.array([0, 20]),                       # past the last train row
                np.array([-1, 3])):
        with pytest.raises(ValueError):
            m.get_self_influence(bad)
    for K in (-1, _lib.FIA_MAX_TOPK + 1, 1.5):
        with pytest.raises(ValueError):
            m.get_self_influence(np.array([1, 2]), K=K)
        with pytest.raises(ValueError):
            m.get_self_influence(None, K=K)
    with pytest.raises(ValueError):
        m.get_self_influence(np.array([1, 2]), K=0, full=False)          # asks for nothing
    with pytest.raises(ValueError):
        m.get_self_influence(None, full=False)
    # what passes the checks: an int32 row array (duplicates kept, in the order given), or None
    rows, K = m._checked_self_rows([19, 3, 3, 0], 4, True)
    assert rows.dtype == np.int32 and rows.tolist() == [19, 3, 3, 0] and K == 4
    rows, K = m._checked_self_rows(np.array([7], np.uint8), _lib.FIA_MAX_TOPK, False)
    assert rows.dtype == np.int32 and rows.tolist() == [7] and K == _lib.FIA_MAX_TOPK
    rows, K = m._checked_self_rows([], 0, True)
    assert rows.dtype == np.int32 and rows.size == 0
    assert m._checked_self_rows(None, 0, True) == (None, 0)


@pytest.mark.parametrize("model,k", [("MF", 8), ("NCF", 8)])
def test_self_reference_identities(model, k):
    p, tu, ti, tr = _problem(model, k)
    W3g = w3g_of(model, p, k)
    seen = []
    for j in (0, 11, len(tr) - 1):
        first, newton, e, cond, core, ref = self_reference(model, p, k, tu, ti, tr, j, WD, DAMP, W3g)
        # first_order: the sum of core["influence"] over the row's two occurrences
        want = core["influence"][ref["occ"]].sum()
        assert abs(first - want) <= 1e-12 * abs(want)
        # the row's own curvature matters: the Newton value is not the first-order one
        assert newton != first and np.isfinite(newton) and np.isfinite(cond)
        seen.append((first, newton, e))
    assert len(set(seen)) == len(seen)


@pytest.mark.parametrize("model,k", [("MF", 8), ("NCF", 8)])
def test_rows_of_a_duplicated_pair_differ(model, k):
    """A pair present twice in train: each of its rows has m = 2 and its own y."""
    p, tu, ti, tr = _problem(model, k)
    tu, ti = np.append(tu, tu[11]), np.append(ti, ti[11])
    tr = np.append(tr, np.float32(tr[11] + 1.5 if tr[11] < 3 else tr[11] - 1.5))
    W3g = w3g_of(model, p, k)
    j0, j1 = 11, len(tr) - 1
    core = fo.query(model, p, k, tu, ti, tr, int(tu[j0]), int(ti[j0]), WD, DAMP)
    out = []
    for j in (j0, j1):
        ref = group_reference(core, [j], WD, DAMP, W3g)
        occ = np.nonzero(core["rel"] == j)[0]
        assert occ.size == 2 and np.array_equal(ref["occ"], occ)             # m = 2 for each row
        want = core["influence"][occ].sum()
        assert abs(ref["first_order"] - want) <= 1e-12 * abs(want)
        out.append((ref["first_order"], ref["group"], float(core["e"][occ[0]])))
    assert out[0][0] != out[1][0] and out[0][1] != out[1][1]
    assert abs((out[0][2] - out[1][2]) - (float(tr[j1]) - float(tr[j0]))) < 1e-12
