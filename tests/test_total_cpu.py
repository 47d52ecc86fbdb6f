"""CPU tests of the total-influence call: fia_total_influence is declared, exported and bound,
refuses a NULL context (whatever the batch size), and the facade validates weights, K and the
inverse_hvp size on the host -- ValueError before any GPU call (the objects here have no GPU
context)."""
import ctypes

import numpy as np
import pytest

from influence import _lib
from influence.NCF import NCF
from influence.matrix_factorization import MF

from test_abi import header_functions


def test_total_influence_declared_exported_bound(libfia_path):
    assert "fia_total_influence" in header_functions()
    assert hasattr(ctypes.CDLL(libfia_path), "fia_total_influence")
    assert "fia_total_influence" in _lib.SIGNATURES
    lib = _lib.load_library(libfia_path)
    assert lib.fia_total_influence(None, 0, None, None, None, None, None, 0, None, None, None) == 1   # FIA_ERR_INVALID
    assert lib.fia_total_influence(None, 2 ** 30 + 1, None, None, None, None, None, 0, None, None, None) == 1
    assert lib.fia_version() == 100


def _bare(cls, k=8, U=7, I=5):
    m = cls.__new__(cls)          # no GPU context: only the host-side validation is exercised
    m.num_users, m.num_items, m.embedding_size = U, I, k
    return m


def _d(cls, k=8):
    return 2 * k + 2 if cls is MF else 4 * k


@pytest.mark.parametrize("cls", [MF, NCF])
def test_total_influence_host_validation(cls):
    m = _bare(cls)
    x = np.zeros((3, _d(cls)))
    for kw in (dict(weights=np.ones(2)),                             # wrong length
               dict(weights=np.ones(4)),
               dict(weights=np.ones((3, 1))),                         # not [Q]
               dict(weights=np.array([1.0, np.nan, 1.0])),            # not finite
               dict(weights=np.array([1.0, np.inf, 1.0])),
               dict(K=-1),
               dict(K=65),
               dict(inverse_hvp=np.zeros((3, _d(cls) + 1))),          # wrong size
               dict(inverse_hvp=np.zeros((2, _d(cls)))),
               dict(weights=np.ones(3), K=65),
               dict(full=False)):                                     # nothing asked for
        kw.setdefault("inverse_hvp", x)
        with pytest.raises(ValueError):
            m.get_total_influence([0, 1, 2], **kw)
