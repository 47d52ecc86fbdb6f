"""CPU tests of the hypothetical-rating ("phantom point") call: fia_score_candidates is
declared, exported and bound, refuses a NULL context, and the facade validates a candidate
batch on the host -- ValueError before any GPU call (the objects here have no GPU context)."""
import ctypes

import numpy as np
import pytest

from influence import _lib
from influence.NCF import NCF
from influence.matrix_factorization import MF

from test_abi import header_functions


def test_score_candidates_declared_exported_bound(libfia_path):
    assert "fia_score_candidates" in header_functions()
    assert hasattr(ctypes.CDLL(libfia_path), "fia_score_candidates")
    assert "fia_score_candidates" in _lib.SIGNATURES
    lib = _lib.load_library(libfia_path)
    rc = lib.fia_score_candidates(None, 0, None, None, None, None, 0, None, None, None, None, 0, None, None, None)
    assert rc == 1          # FIA_ERR_INVALID
    assert lib.fia_version() == 100


def _bare(cls, U=7, I=5):
    m = cls.__new__(cls)          # no GPU context: only the host-side validation is exercised
    m.num_users, m.num_items = U, I
    return m


GOOD_X = np.array([[0, 0], [6, 4], [3, 2]], np.int64)
GOOD_Y = np.array([1.5, 2.5, 3.5])


@pytest.mark.parametrize("cls", [MF, NCF])
@pytest.mark.parametrize("offsets,X,Y", [
    ([0, 2], GOOD_X, GOOD_Y),                                    # does not end at M
    ([1, 3], GOOD_X, GOOD_Y),                                    # does not start at 0
    ([0, 3, 3], GOOD_X, GOOD_Y),                                 # Q + 1 values wanted, 3 given for 1 query
    ([0, 3], GOOD_X, GOOD_Y[:2]),                                # X / Y length mismatch
    ([0, 3], np.array([[0, 0], [7, 4], [3, 2]]), GOOD_Y),        # user id == U
    ([0, 3], np.array([[0, 0], [6, 5], [3, 2]]), GOOD_Y),        # item id == I
    ([0, 3], np.array([[0, 0], [-1, 4], [3, 2]]), GOOD_Y),       # negative id
    ([0, 3], np.array([[0, 0], [6, -2], [3, 2]]), GOOD_Y),
    ([0, 3], GOOD_X.reshape(-1), GOOD_Y),                        # X not [M, 2]
])
def test_candidate_batch_host_validation(cls, offsets, X, Y):
    m = _bare(cls)
    with pytest.raises(ValueError):
        m.get_candidate_influence_batch([0], np.array(offsets, np.int64), X, Y)


@pytest.mark.parametrize("cls", [MF, NCF])
def test_candidate_batch_offsets_must_not_decrease(cls):
    m = _bare(cls)
    with pytest.raises(ValueError):
        m.get_candidate_influence_batch([0, 1, 2], np.array([0, 2, 1, 3], np.int64), GOOD_X, GOOD_Y)


@pytest.mark.parametrize("cls", [MF, NCF])
def test_phantom_single_query_validates_before_gpu(cls):
    """get_influence_on_test_loss(train_idx=None, X, Y): the reference's ValueErrors stay, and
    an out-of-range candidate id is a ValueError raised before any GPU call."""
    m = _bare(cls)
    with pytest.raises(ValueError):
        m.get_influence_on_test_loss([0], None)
    with pytest.raises(ValueError):
        m.get_influence_on_test_loss([0], None, X=GOOD_X, Y=GOOD_Y[:2])
    with pytest.raises(ValueError):
        m.get_influence_on_test_loss([0], np.arange(3), X=GOOD_X, Y=GOOD_Y)
    with pytest.raises(ValueError):
        m.get_influence_on_test_loss([0], None, X=np.array([[7, 0]]), Y=np.array([1.0]))
