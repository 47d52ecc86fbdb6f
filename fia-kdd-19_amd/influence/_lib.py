"""ctypes binding of libfia.so (include/fia.h) for torch device tensors.

This is the ONLY compute path of the package: there is no CPU fallback.  If
the library is missing (not built) or no GPU is visible, every entry point
raises, loudly.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FIA_LIB", os.path.join(_HERE, "libfia.so"))

FIA_OK = 0
FIA_MODEL_MF = 0
FIA_MODEL_NCF = 1
FIA_MAX_TOPK = 64
FIA_SLATE_MAX_ITEMS = 64
FIA_NUM_PHASES = 5
FIA_FLIP_MAX_SET = 64
PHASES = ("prepare", "solve", "score", "topk", "chunks")

_ERR = {1: "invalid argument", 2: "HIP error", 3: "bad call order", 4: "unsupported", 5: "out of memory"}

# exported symbol -> (restype, argtypes); every symbol declared in include/fia.h
_P = ctypes.c_void_p
_I64 = ctypes.c_int64
SIGNATURES = {
    "fia_version": (ctypes.c_int, []),
    "fia_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_P)]),
    "fia_destroy": (ctypes.c_int, [_P]),
    "fia_last_error": (ctypes.c_char_p, [_P]),
    "fia_set_params": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _I64, _I64, ctypes.POINTER(_P), ctypes.c_int,
                                      ctypes.c_double, ctypes.c_double]),
    "fia_build_index": (ctypes.c_int, [_P, _I64, _I64, _I64, _P, _P, _P, _P]),
    "fia_prepare": (ctypes.c_int, [_P, _P]),
    "fia_prepare_for": (ctypes.c_int, [_P, _I64, _P, _P, _P]),
    "fia_count_related": (ctypes.c_int, [_P, _I64, _P, _P, _P, ctypes.POINTER(_I64), _P]),
    "fia_related": (ctypes.c_int, [_P, _I64, _P, _P, _P, _P, _P]),
    "fia_query_batch": (ctypes.c_int, [_P, _I64, _P, _P, _P, _I64, _P, _P, _P, ctypes.c_int, _P, _P, _P, _P]),
    "fia_query_batch_x": (ctypes.c_int, [_P, _I64, _P, _P, _P, _I64, _P, _P, _P, ctypes.c_int, _P, _P, _P, _P]),
    "fia_score_candidates": (ctypes.c_int, [_P, _I64, _P, _P, _P, _P, _I64, _P, _P, _P, _P, ctypes.c_int, _P, _P, _P]),
    "fia_total_influence": (ctypes.c_int, [_P, _I64, _P, _P, _P, _P, _P, ctypes.c_int, _P, _P, _P]),
    "fia_group_influence": (ctypes.c_int, [_P, _I64, _P, _P, _P, _I64, _P, _I64, _P, _P, _P, _P, _P]),
    "fia_self_influence": (ctypes.c_int, [_P, _I64, _P, _P, _P, _P, ctypes.c_int, _P, _P, _P, _P]),
    "fia_query_batch_newton": (ctypes.c_int, [_P, _I64, _P, _P, _P, _I64, _P, _P, ctypes.c_int, _P, _P, _P, _P]),
    "fia_score_candidates_newton": (ctypes.c_int, [_P, _I64, _P, _P, _P, _I64, _P, _P, _P, _P, ctypes.c_int, _P, _P,
                                                   _P]),
    "fia_edit_influence": (ctypes.c_int, [_P, _I64, _P, _P, _P, _I64, _P, _I64, _P, _P, _I64, _P, _P, _P, _P, _P, _P,
                                          ctypes.c_int, _P, _P, _P]),
    "fia_count_related_pair": (ctypes.c_int, [_P, _I64, _P, _P, _P, _P, ctypes.POINTER(_I64), _P]),
    "fia_pair_batch": (ctypes.c_int, [_P, _I64, _P, _P, _P, _P, _I64, _P, _P, _P, _P, ctypes.c_int, _P, _P, _P, _P]),
    "fia_pair_flip": (ctypes.c_int, [_P, _I64, _P, _P, _P, _P, ctypes.c_int, _P, _P, _P, _P, _P, _P, _P, _P]),
    "fia_count_related_slate": (ctypes.c_int, [_P, _I64, _P, _P, _I64, _P, _P, ctypes.POINTER(_I64), _P]),
    "fia_slate_batch": (ctypes.c_int, [_P, _I64, _P, _P, _I64, _P, _P, _P, _I64, _P, _P, _P, _P, ctypes.c_int, _P, _P,
                                       _P, _P]),
    "fia_num_params": (ctypes.c_int, [_P]),
    "fia_set_profiling": (ctypes.c_int, [_P, ctypes.c_int]),
    "fia_profile_read": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_I64)]),
}

_lib = None


class FIAError(RuntimeError):
    pass


def load_library(path=None):
    """dlopen libfia.so and bind every symbol (no GPU needed for this step)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ImportError("FIA HIP library not built: %s is missing (run __graft_entry__.build() or "
                          "make -C fia-kdd-19_amd/csrc)" % p)
    lib = ctypes.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Context(object):
    """One fia_ctx bound to one HIP device."""

    def __init__(self, device=0):
        import torch
        if not torch.cuda.is_available():
            raise FIAError("FIA needs a ROCm GPU: torch.cuda.is_available() is False (no CPU fallback)")
        self.lib = load_library()
        self.device = device
        self.torch_device = torch.device("cuda", device)
        h = ctypes.c_void_p()
        rc = self.lib.fia_create(device, ctypes.byref(h))
        if rc != FIA_OK:
            raise FIAError("fia_create(%d) failed: %s" % (device, _ERR.get(rc, rc)))
        self.h = h
        self._keep = []
        self._mask = 0
        self._carry = None      # phase sums drained by profiled_call on the caller's behalf
        self.full_prepared = False   # every entity's caches (the last prepare was fia_prepare)

    def close(self):
        if getattr(self, "h", None):
            self.lib.fia_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != FIA_OK:
            msg = self.lib.fia_last_error(self.h)
            raise FIAError("%s failed (%s): %s" % (what, _ERR.get(rc, rc), msg.decode() if msg else ""))

    # ---- setup ----
    def set_params(self, model, k, U, I, tables, wd, damping):
        """tables: list of contiguous float32 cuda tensors in include/fia.h order."""
        arr = (ctypes.c_void_p * len(tables))(*[t.data_ptr() for t in tables])
        self._keep = list(tables)
        self.full_prepared = False
        self._num_params = None
        rc = self.lib.fia_set_params(self.h, model, k, U, I, arr, len(tables), float(wd), float(damping))
        self._check(rc, "fia_set_params")

    def build_index(self, users, items, ratings, U, I):
        self.full_prepared = False
        rc = self.lib.fia_build_index(self.h, users.numel(), U, I, _ptr(users), _ptr(items), _ptr(ratings),
                                      _stream())
        self._check(rc, "fia_build_index")
        self.n_train = users.numel()

    def prepare(self):
        self.full_prepared = False
        self._check(self.lib.fia_prepare(self.h, _stream()), "fia_prepare")
        self.full_prepared = True

    def prepare_for(self, qu, qi):
        """Hessian caches for only the users/items of these queries (fia_prepare_for, every
        model: small k marks the entities on the device, large k builds a compact cache)."""
        self.full_prepared = False
        self._check(self.lib.fia_prepare_for(self.h, qu.numel(), _ptr(qu), _ptr(qi), _stream()), "fia_prepare_for")

    def num_params(self):
        if getattr(self, "_num_params", None) is None:
            self._num_params = self.lib.fia_num_params(self.h)
        return self._num_params

    # ---- queries ----
    def count_related(self, qu, qi, offsets=None, want_total=True):
        import torch
        Q = qu.numel()
        if offsets is None:
            offsets = torch.empty(Q + 1, dtype=torch.int64, device=self.torch_device)
        total = ctypes.c_int64(0)
        rc = self.lib.fia_count_related(self.h, Q, _ptr(qu), _ptr(qi), _ptr(offsets),
                                        ctypes.byref(total) if want_total else None, _stream())
        self._check(rc, "fia_count_related")
        return offsets, (total.value if want_total else None)

    @staticmethod
    def _need_int32(t, name):
        # the library writes train rows as int32 (include/fia.h fia_related)
        import torch
        if t is not None and t.dtype != torch.int32:
            raise TypeError("%s must be a torch.int32 tensor (got %s)" % (name, t.dtype))

    def related(self, qu, qi, offsets, rel_idx):
        self._need_int32(rel_idx, "rel_idx")
        rc = self.lib.fia_related(self.h, qu.numel(), _ptr(qu), _ptr(qi), _ptr(offsets), _ptr(rel_idx), _stream())
        self._check(rc, "fia_related")

    def query_batch(self, qu, qi, offsets, total, rel_idx=None, influence=None, x=None, K=0,
                    topk_pos=None, topk_idx=None, topk_val=None):
        self._need_int32(rel_idx, "rel_idx")
        rc = self.lib.fia_query_batch(self.h, qu.numel(), _ptr(qu), _ptr(qi), _ptr(offsets), int(total),
                                      _ptr(rel_idx), _ptr(influence), _ptr(x), int(K), _ptr(topk_pos),
                                      _ptr(topk_idx), _ptr(topk_val), _stream())
        self._check(rc, "fia_query_batch")

    def query_batch_x(self, qu, qi, offsets, total, x_in, rel_idx=None, influence=None, K=0,
                      topk_pos=None, topk_idx=None, topk_val=None):
        """fia_query_batch with the given inverse HVPs x_in (float64 cuda tensor [Q * D],
        reference theta order) instead of the solve."""
        import torch
        self._need_int32(rel_idx, "rel_idx")
        if x_in.dtype != torch.float64 or not x_in.is_contiguous():
            raise TypeError("x_in must be a contiguous torch.float64 tensor")
        if not x_in.is_cuda:
            raise TypeError("x_in must be a device (cuda) tensor")
        if x_in.numel() < qu.numel() * self.num_params():
            raise ValueError("x_in holds %d values, %d queries need %d" % (
                x_in.numel(), qu.numel(), qu.numel() * self.num_params()))
        rc = self.lib.fia_query_batch_x(self.h, qu.numel(), _ptr(qu), _ptr(qi), _ptr(offsets), int(total),
                                        _ptr(x_in), _ptr(rel_idx), _ptr(influence), int(K), _ptr(topk_pos),
                                        _ptr(topk_idx), _ptr(topk_val), _stream())
        self._check(rc, "fia_query_batch_x")

    def score_candidates(self, qu, qi, x, cand_offsets, total, cand_user, cand_item, cand_rating,
                         influence=None, K=0, topk_pos=None, topk_val=None):
        """fia_score_candidates: the influence of hypothetical ratings (cand_user, cand_item,
        cand_rating), candidates cand_offsets[q]:cand_offsets[q+1] belonging to query q, given
        the queries' inverse HVPs x (float64 cuda tensor [Q * D], reference theta order)."""
        import torch
        for t, name in ((qu, "qu"), (qi, "qi"), (cand_user, "cand_user"), (cand_item, "cand_item")):
            self._need_int32(t, name)
        if x.dtype != torch.float64 or not x.is_contiguous() or not x.is_cuda:
            raise TypeError("x must be a contiguous torch.float64 device (cuda) tensor")
        if x.numel() < qu.numel() * self.num_params():
            raise ValueError("x holds %d values, %d queries need %d" % (
                x.numel(), qu.numel(), qu.numel() * self.num_params()))
        if cand_rating.dtype != torch.float32:
            raise TypeError("cand_rating must be a torch.float32 tensor (got %s)" % cand_rating.dtype)
        if cand_offsets.dtype != torch.int64 or cand_offsets.numel() != qu.numel() + 1:
            raise TypeError("cand_offsets must be a torch.int64 tensor of Q + 1 values")
        if influence is not None and influence.dtype != torch.float64:
            raise TypeError("influence must be a torch.float64 tensor")
        if topk_pos is not None and topk_pos.dtype != torch.int64:
            raise TypeError("topk_pos must be a torch.int64 tensor")
        if topk_val is not None and topk_val.dtype != torch.float64:
            raise TypeError("topk_val must be a torch.float64 tensor")
        for t, name in ((cand_offsets, "cand_offsets"), (cand_user, "cand_user"), (cand_item, "cand_item"),
                        (cand_rating, "cand_rating"), (influence, "influence"), (topk_pos, "topk_pos"),
                        (topk_val, "topk_val")):
            if t is not None and not (t.is_cuda and t.is_contiguous()):
                raise TypeError("%s must be a contiguous device (cuda) tensor" % name)
        if min(cand_user.numel(), cand_item.numel(), cand_rating.numel()) < total or (
                influence is not None and influence.numel() < total):
            raise ValueError("candidate arrays hold fewer than total = %d values" % total)
        if K and (topk_pos is None or topk_val is None or min(topk_pos.numel(), topk_val.numel()) < qu.numel() * K):
            raise ValueError("top-K outputs must hold Q * K values")
        rc = self.lib.fia_score_candidates(self.h, qu.numel(), _ptr(qu), _ptr(qi), _ptr(x), _ptr(cand_offsets),
                                           int(total), _ptr(cand_user), _ptr(cand_item), _ptr(cand_rating),
                                           _ptr(influence), int(K), _ptr(topk_pos), _ptr(topk_val), _stream())
        self._check(rc, "fia_score_candidates")

    def total_influence(self, qu, qi, x, total=None, count=None, K=0, topk_idx=None, topk_val=None):
        """fia_total_influence: for every train row the sum of its influence on the queries
        (qu, qi) with inverse HVPs x (float64 cuda tensor [Q * D], reference theta order) --
        the scatter-add of query_batch_x's influence by rel_idx -- into total (float64
        [n_train]) and count (int32 [n_train]); with K the K rows of largest |total| (topk_idx
        int64 [K], topk_val float64 [K]).  n_train is the size of the built index: total and
        count, when given, must hold that many values."""
        import torch
        self._need_int32(qu, "qu")
        self._need_int32(qi, "qi")
        self._need_int32(count, "count")
        if qi.numel() != qu.numel():
            raise ValueError("qu and qi must have the same length")
        if x.dtype != torch.float64 or not x.is_contiguous() or not x.is_cuda:
            raise TypeError("x must be a contiguous torch.float64 device (cuda) tensor")
        if x.numel() < qu.numel() * self.num_params():
            raise ValueError("x holds %d values, %d queries need %d" % (
                x.numel(), qu.numel(), qu.numel() * self.num_params()))
        if total is not None and total.dtype != torch.float64:
            raise TypeError("total must be a torch.float64 tensor")
        if topk_idx is not None and topk_idx.dtype != torch.int64:
            raise TypeError("topk_idx must be a torch.int64 tensor")
        if topk_val is not None and topk_val.dtype != torch.float64:
            raise TypeError("topk_val must be a torch.float64 tensor")
        for t, name in ((qu, "qu"), (qi, "qi"), (total, "total"), (count, "count"), (topk_idx, "topk_idx"),
                        (topk_val, "topk_val")):
            if t is not None and not (t.is_cuda and t.is_contiguous()):
                raise TypeError("%s must be a contiguous device (cuda) tensor" % name)
        n_train = getattr(self, "n_train", None)
        for t, name in ((total, "total"), (count, "count")):
            if t is not None and n_train is not None and t.numel() < n_train:
                raise ValueError("%s holds %d values, the index has %d train rows" % (name, t.numel(), n_train))
        if K and (topk_idx is None or topk_val is None or min(topk_idx.numel(), topk_val.numel()) < K):
            raise ValueError("top-K outputs must hold K values")
        rc = self.lib.fia_total_influence(self.h, qu.numel(), _ptr(qu), _ptr(qi), _ptr(x), _ptr(total), _ptr(count),
                                          int(K), _ptr(topk_idx), _ptr(topk_val), _stream())
        self._check(rc, "fia_total_influence")

    def group_influence(self, qu, qi, grp_offsets, mem_offsets, mem_row, group=None, first_order=None,
                        dtheta=None):
        """fia_group_influence: for every group of train rows (group g of query q for g in
        grp_offsets[q]:grp_offsets[q+1], its members mem_row[mem_offsets[g]:mem_offsets[g+1]])
        the predicted change of r-hat when the rows are removed together -- the system with the
        rows' terms taken out, solved again -- into group (float64 [G]), the sum of the rows'
        single-rating influences into first_order (float64 [G]) and the parameter step into
        dtheta (float64 [G * D], reference theta order).  Offsets are int64, rows int32."""
        import torch
        for t, name in ((qu, "qu"), (qi, "qi"), (mem_row, "mem_row")):
            self._need_int32(t, name)
        if qi.numel() != qu.numel():
            raise ValueError("qu and qi must have the same length")
        Q = qu.numel()
        if grp_offsets.dtype != torch.int64 or grp_offsets.numel() != Q + 1:
            raise TypeError("grp_offsets must be a torch.int64 tensor of Q + 1 values")
        if mem_offsets.dtype != torch.int64 or mem_offsets.numel() < 1:
            raise TypeError("mem_offsets must be a torch.int64 tensor of G + 1 values")
        G = mem_offsets.numel() - 1
        for t, name in ((group, "group"), (first_order, "first_order"), (dtheta, "dtheta")):
            if t is not None and t.dtype != torch.float64:
                raise TypeError("%s must be a torch.float64 tensor" % name)
        for t, name in ((qu, "qu"), (qi, "qi"), (grp_offsets, "grp_offsets"), (mem_offsets, "mem_offsets"),
                        (mem_row, "mem_row"), (group, "group"), (first_order, "first_order"), (dtheta, "dtheta")):
            if t is not None and not (t.is_cuda and t.is_contiguous()):
                raise TypeError("%s must be a contiguous device (cuda) tensor" % name)
        if group is None and first_order is None and dtheta is None:
            raise ValueError("no output requested (group, first_order, dtheta)")
        for t, name in ((group, "group"), (first_order, "first_order")):
            if t is not None and t.numel() < G:
                raise ValueError("%s holds %d values, the batch has %d groups" % (name, t.numel(), G))
        if dtheta is not None and dtheta.numel() < G * self.num_params():
            raise ValueError("dtheta holds %d values, %d groups need %d" % (
                dtheta.numel(), G, G * self.num_params()))
        total = mem_row.numel() if mem_row is not None else 0
        rc = self.lib.fia_group_influence(self.h, Q, _ptr(qu), _ptr(qi), _ptr(grp_offsets), G, _ptr(mem_offsets),
                                          total, _ptr(mem_row), _ptr(group), _ptr(first_order), _ptr(dtheta),
                                          _stream())
        self._check(rc, "fia_group_influence")

    def self_influence(self, rows=None, first_order=None, newton=None, error=None, K=0, topk_pos=None,
                       topk_idx=None, topk_val=None):
        """fia_self_influence: for every train row listed in rows (int32; None = every row of the
        built index, in order) its effect on its own prediction -- first_order, the sum of its two
        influences in its own related list; newton, the same with the row's curvature taken out of
        the system; error = r-hat - y (float64 [num_rows] each, any may be None) -- and with K
        the K positions of largest |newton| (topk_pos / topk_idx int64 [K], topk_val float64
        [K]).  A row outside [0, n_train) gives NaN."""
        import torch
        self._need_int32(rows, "rows")
        n_train = getattr(self, "n_train", None)
        if rows is None and n_train is None:
            raise FIAError("self_influence(rows=None) needs a built index")
        n = n_train if rows is None else rows.numel()
        for t, name in ((first_order, "first_order"), (newton, "newton"), (error, "error"), (topk_val, "topk_val")):
            if t is not None and t.dtype != torch.float64:
                raise TypeError("%s must be a torch.float64 tensor" % name)
        for t, name in ((topk_pos, "topk_pos"), (topk_idx, "topk_idx")):
            if t is not None and t.dtype != torch.int64:
                raise TypeError("%s must be a torch.int64 tensor" % name)
        for t, name in ((rows, "rows"), (first_order, "first_order"), (newton, "newton"), (error, "error"),
                        (topk_pos, "topk_pos"), (topk_idx, "topk_idx"), (topk_val, "topk_val")):
            if t is not None and not (t.is_cuda and t.is_contiguous()):
                raise TypeError("%s must be a contiguous device (cuda) tensor" % name)
        for t, name in ((first_order, "first_order"), (newton, "newton"), (error, "error")):
            if t is not None and t.numel() < n:
                raise ValueError("%s holds %d values, the batch has %d rows" % (name, t.numel(), n))
        if K and (topk_pos is None or topk_idx is None or topk_val is None
                  or min(topk_pos.numel(), topk_idx.numel(), topk_val.numel()) < K):
            raise ValueError("top-K outputs must hold K values")
        rc = self.lib.fia_self_influence(self.h, n, _ptr(rows), _ptr(first_order), _ptr(newton), _ptr(error), int(K),
                                         _ptr(topk_pos), _ptr(topk_idx), _ptr(topk_val), _stream())
        self._check(rc, "fia_self_influence")

    def query_batch_newton(self, qu, qi, offsets, total, rel_idx=None, newton=None, K=0, topk_pos=None,
                           topk_idx=None, topk_val=None):
        """fia_query_batch_newton: for every related rating of every query its Newton-corrected
        influence -- the system without that rating's curvature, one factorisation per query --
        into newton (float64 [total]), the train rows into rel_idx (int32 [total]), and with K the
        K related ratings of largest |newton| per query (topk_pos / topk_idx int64 [Q * K],
        topk_val float64 [Q * K]).  offsets / total as count_related returns them."""
        import torch
        for t, name in ((qu, "qu"), (qi, "qi"), (rel_idx, "rel_idx")):
            self._need_int32(t, name)
        if qi.numel() != qu.numel():
            raise ValueError("qu and qi must have the same length")
        Q = qu.numel()
        if offsets.dtype != torch.int64 or offsets.numel() != Q + 1:
            raise TypeError("offsets must be a torch.int64 tensor of Q + 1 values")
        for t, name in ((newton, "newton"), (topk_val, "topk_val")):
            if t is not None and t.dtype != torch.float64:
                raise TypeError("%s must be a torch.float64 tensor" % name)
        for t, name in ((topk_pos, "topk_pos"), (topk_idx, "topk_idx")):
            if t is not None and t.dtype != torch.int64:
                raise TypeError("%s must be a torch.int64 tensor" % name)
        for t, name in ((qu, "qu"), (qi, "qi"), (offsets, "offsets"), (rel_idx, "rel_idx"), (newton, "newton"),
                        (topk_pos, "topk_pos"), (topk_idx, "topk_idx"), (topk_val, "topk_val")):
            if t is not None and not (t.is_cuda and t.is_contiguous()):
                raise TypeError("%s must be a contiguous device (cuda) tensor" % name)
        for t, name in ((rel_idx, "rel_idx"), (newton, "newton")):
            if t is not None and t.numel() < total:
                raise ValueError("%s holds %d values, the batch has %d related ratings" % (name, t.numel(), total))
        if K and (topk_pos is None or topk_idx is None or topk_val is None
                  or min(topk_pos.numel(), topk_idx.numel(), topk_val.numel()) < Q * K):
            raise ValueError("top-K outputs must hold Q * K values")
        rc = self.lib.fia_query_batch_newton(self.h, Q, _ptr(qu), _ptr(qi), _ptr(offsets), int(total), _ptr(rel_idx),
                                             _ptr(newton), int(K), _ptr(topk_pos), _ptr(topk_idx), _ptr(topk_val),
                                             _stream())
        self._check(rc, "fia_query_batch_newton")

    def score_candidates_newton(self, qu, qi, cand_offsets, total, cand_user, cand_item, cand_rating,
                                newton_add=None, K=0, topk_pos=None, topk_val=None):
        """fia_score_candidates_newton: the Newton-corrected influence of hypothetical ratings
        (cand_user, cand_item, cand_rating), candidates cand_offsets[q]:cand_offsets[q+1] belonging
        to query q -- score_candidates with the candidate's own curvature in the system, one
        factorisation per query (no x is passed) -- into newton_add (float64 [total]) and, with K,
        the K candidates of largest |newton_add| per query (topk_pos int64 [Q * K] positions inside
        the query's list, topk_val float64 [Q * K])."""
        import torch
        for t, name in ((qu, "qu"), (qi, "qi"), (cand_user, "cand_user"), (cand_item, "cand_item")):
            self._need_int32(t, name)
        if qi.numel() != qu.numel():
            raise ValueError("qu and qi must have the same length")
        Q = qu.numel()
        if cand_rating.dtype != torch.float32:
            raise TypeError("cand_rating must be a torch.float32 tensor (got %s)" % cand_rating.dtype)
        if cand_offsets.dtype != torch.int64 or cand_offsets.numel() != Q + 1:
            raise TypeError("cand_offsets must be a torch.int64 tensor of Q + 1 values")
        for t, name in ((newton_add, "newton_add"), (topk_val, "topk_val")):
            if t is not None and t.dtype != torch.float64:
                raise TypeError("%s must be a torch.float64 tensor" % name)
        if topk_pos is not None and topk_pos.dtype != torch.int64:
            raise TypeError("topk_pos must be a torch.int64 tensor")
        for t, name in ((qu, "qu"), (qi, "qi"), (cand_offsets, "cand_offsets"), (cand_user, "cand_user"),
                        (cand_item, "cand_item"), (cand_rating, "cand_rating"), (newton_add, "newton_add"),
                        (topk_pos, "topk_pos"), (topk_val, "topk_val")):
            if t is not None and not (t.is_cuda and t.is_contiguous()):
                raise TypeError("%s must be a contiguous device (cuda) tensor" % name)
        if min(cand_user.numel(), cand_item.numel(), cand_rating.numel()) < total or (
                newton_add is not None and newton_add.numel() < total):
            raise ValueError("candidate arrays hold fewer than total = %d values" % total)
        if K and (topk_pos is None or topk_val is None or min(topk_pos.numel(), topk_val.numel()) < Q * K):
            raise ValueError("top-K outputs must hold Q * K values")
        rc = self.lib.fia_score_candidates_newton(self.h, Q, _ptr(qu), _ptr(qi), _ptr(cand_offsets), int(total),
                                                  _ptr(cand_user), _ptr(cand_item), _ptr(cand_rating),
                                                  _ptr(newton_add), int(K), _ptr(topk_pos), _ptr(topk_val), _stream())
        self._check(rc, "fia_score_candidates_newton")

    def edit_influence(self, qu, qi, grp_offsets, rem_offsets, rem_row, add_offsets, add_user, add_item,
                       add_rating, edit=None, first_order=None, dtheta=None, K=0, topk_pos=None, topk_val=None):
        """fia_edit_influence: for every edit set (group g of query q for g in
        grp_offsets[q]:grp_offsets[q+1]; its removals rem_row[rem_offsets[g]:rem_offsets[g+1]],
        train rows, and its additions add_offsets[g]:add_offsets[g+1] of add_user / add_item /
        add_rating) the predicted change of r-hat once the rows are removed and the ratings added
        together -- one system per group, solved again -- into edit (float64 [G]), its
        first-order counterpart into first_order (float64 [G]) and the parameter step into dtheta
        (float64 [G * D], reference theta order); with K the K groups of largest |edit| per query
        (topk_pos int64 [Q * K] positions inside the query, topk_val float64 [Q * K]).  Offsets
        are int64, rows and ids int32, ratings float32."""
        import torch
        for t, name in ((qu, "qu"), (qi, "qi"), (rem_row, "rem_row"), (add_user, "add_user"), (add_item, "add_item")):
            self._need_int32(t, name)
        if qi.numel() != qu.numel():
            raise ValueError("qu and qi must have the same length")
        Q = qu.numel()
        if grp_offsets.dtype != torch.int64 or grp_offsets.numel() != Q + 1:
            raise TypeError("grp_offsets must be a torch.int64 tensor of Q + 1 values")
        for t, name in ((rem_offsets, "rem_offsets"), (add_offsets, "add_offsets")):
            if t.dtype != torch.int64 or t.numel() < 1:
                raise TypeError("%s must be a torch.int64 tensor of G + 1 values" % name)
        G = rem_offsets.numel() - 1
        if add_offsets.numel() != G + 1:
            raise ValueError("rem_offsets and add_offsets must have the same length")
        if add_rating is not None and add_rating.dtype != torch.float32:
            raise TypeError("add_rating must be a torch.float32 tensor (got %s)" % add_rating.dtype)
        for t, name in ((edit, "edit"), (first_order, "first_order"), (dtheta, "dtheta"), (topk_val, "topk_val")):
            if t is not None and t.dtype != torch.float64:
                raise TypeError("%s must be a torch.float64 tensor" % name)
        if topk_pos is not None and topk_pos.dtype != torch.int64:
            raise TypeError("topk_pos must be a torch.int64 tensor")
        for t, name in ((qu, "qu"), (qi, "qi"), (grp_offsets, "grp_offsets"), (rem_offsets, "rem_offsets"),
                        (rem_row, "rem_row"), (add_offsets, "add_offsets"), (add_user, "add_user"),
                        (add_item, "add_item"), (add_rating, "add_rating"), (edit, "edit"),
                        (first_order, "first_order"), (dtheta, "dtheta"), (topk_pos, "topk_pos"),
                        (topk_val, "topk_val")):
            if t is not None and not (t.is_cuda and t.is_contiguous()):
                raise TypeError("%s must be a contiguous device (cuda) tensor" % name)
        K = int(K)
        if edit is None and first_order is None and dtheta is None and K == 0:
            raise ValueError("no output requested (edit, first_order, dtheta, top-K)")
        for t, name in ((edit, "edit"), (first_order, "first_order")):
            if t is not None and t.numel() < G:
                raise ValueError("%s holds %d values, the batch has %d groups" % (name, t.numel(), G))
        if dtheta is not None and dtheta.numel() < G * self.num_params():
            raise ValueError("dtheta holds %d values, %d groups need %d" % (
                dtheta.numel(), G, G * self.num_params()))
        total_rem = rem_row.numel() if rem_row is not None else 0
        total_add = add_user.numel() if add_user is not None else 0
        if total_add and (add_item is None or add_rating is None
                          or min(add_item.numel(), add_rating.numel()) < total_add):
            raise ValueError("addition arrays hold fewer than total_add = %d values" % total_add)
        if K and (topk_pos is None or topk_val is None or min(topk_pos.numel(), topk_val.numel()) < Q * K):
            raise ValueError("top-K outputs must hold Q * K values")
        rc = self.lib.fia_edit_influence(self.h, Q, _ptr(qu), _ptr(qi), _ptr(grp_offsets), G, _ptr(rem_offsets),
                                         total_rem, _ptr(rem_row), _ptr(add_offsets), total_add, _ptr(add_user),
                                         _ptr(add_item), _ptr(add_rating), _ptr(edit), _ptr(first_order),
                                         _ptr(dtheta), K, _ptr(topk_pos), _ptr(topk_val), _stream())
        self._check(rc, "fia_edit_influence")

    def count_related_pair(self, qu, qi, qj, offsets=None, want_total=True):
        """fia_count_related_pair: offsets (int64 [Q + 1]) of the pair queries' related lists
        R_u ++ C_i ++ C_j and, with want_total, their total on the host (then out-of-range ids and
        entities outside a prepare_for cover raise)."""
        import torch
        for t, name in ((qu, "qu"), (qi, "qi"), (qj, "qj")):
            self._need_int32(t, name)
        Q = qu.numel()
        if qi.numel() != Q or qj.numel() != Q:
            raise ValueError("qu, qi and qj must have the same length")
        if offsets is None:
            offsets = torch.empty(Q + 1, dtype=torch.int64, device=self.torch_device)
        total = ctypes.c_int64(0)
        rc = self.lib.fia_count_related_pair(self.h, Q, _ptr(qu), _ptr(qi), _ptr(qj), _ptr(offsets),
                                             ctypes.byref(total) if want_total else None, _stream())
        self._check(rc, "fia_count_related_pair")
        return offsets, (total.value if want_total else None)

    def pair_batch(self, qu, qi, qj, offsets, total, rel_idx=None, influence=None, x=None, diff=None, K=0,
                   topk_pos=None, topk_idx=None, topk_val=None):
        """fia_pair_batch: for every pair query (qu, qi, qj) the influence of every rating of
        R_u ++ C_i ++ C_j on the gap r-hat(u, i) - r-hat(u, j) -- one system over (theta_u, theta_i,
        theta_j), solved once -- into influence (float64 [total]), the train rows into rel_idx
        (int32 [total]), x = H^-1 v into x (float64 [Q * 3 * D / 2], the extended reference theta
        order), the gap into diff (float64 [Q]) and, with K, the K ratings of largest |influence|
        per query (topk_pos / topk_idx int64 [Q * K], topk_val float64 [Q * K]).  offsets / total as
        count_related_pair returns them."""
        import torch
        for t, name in ((qu, "qu"), (qi, "qi"), (qj, "qj"), (rel_idx, "rel_idx")):
            self._need_int32(t, name)
        Q = qu.numel()
        if qi.numel() != Q or qj.numel() != Q:
            raise ValueError("qu, qi and qj must have the same length")
        if offsets.dtype != torch.int64 or offsets.numel() != Q + 1:
            raise TypeError("offsets must be a torch.int64 tensor of Q + 1 values")
        for t, name in ((influence, "influence"), (x, "x"), (diff, "diff"), (topk_val, "topk_val")):
            if t is not None and t.dtype != torch.float64:
                raise TypeError("%s must be a torch.float64 tensor" % name)
        for t, name in ((topk_pos, "topk_pos"), (topk_idx, "topk_idx")):
            if t is not None and t.dtype != torch.int64:
                raise TypeError("%s must be a torch.int64 tensor" % name)
        for t, name in ((qu, "qu"), (qi, "qi"), (qj, "qj"), (offsets, "offsets"), (rel_idx, "rel_idx"),
                        (influence, "influence"), (x, "x"), (diff, "diff"), (topk_pos, "topk_pos"),
                        (topk_idx, "topk_idx"), (topk_val, "topk_val")):
            if t is not None and not (t.is_cuda and t.is_contiguous()):
                raise TypeError("%s must be a contiguous device (cuda) tensor" % name)
        # (an oversized total is the library's to refuse, before it looks at any array)
        if 0 <= total < 2 ** 31:
            for t, name in ((rel_idx, "rel_idx"), (influence, "influence")):
                if t is not None and t.numel() < total:
                    raise ValueError("%s holds %d values, the batch has %d related ratings" % (name, t.numel(), total))
        if x is not None and x.numel() < Q * (3 * self.num_params() // 2):
            raise ValueError("x holds %d values, %d queries need %d" % (x.numel(), Q, Q * (3 * self.num_params() // 2)))
        if diff is not None and diff.numel() < Q:
            raise ValueError("diff holds %d values, the batch has %d queries" % (diff.numel(), Q))
        K = int(K)
        if K > 0 and (topk_pos is None or topk_idx is None or topk_val is None
                      or min(topk_pos.numel(), topk_idx.numel(), topk_val.numel()) < Q * K):
            raise ValueError("top-K outputs must hold Q * K values")
        rc = self.lib.fia_pair_batch(self.h, Q, _ptr(qu), _ptr(qi), _ptr(qj), _ptr(offsets), int(total),
                                     _ptr(rel_idx), _ptr(influence), _ptr(x), _ptr(diff), K, _ptr(topk_pos),
                                     _ptr(topk_idx), _ptr(topk_val), _stream())
        self._check(rc, "fia_pair_batch")

    def pair_flip(self, qu, qi, qj, max_set, margin=None, set_size=None, set_row=None, set_val=None,
                  first_order=None, newton=None, dtheta=None, diff=None):
        """fia_pair_flip: for every pair query (qu, qi, qj) the greedy first-order set of the user's
        own ratings that puts j above i -- the most negative values of R_u, taken while
        diff + margin + their running sum >= 0 and fewer than max_set are taken -- into set_size
        (int32 [Q]), set_row (int32 [Q * max_set] train rows, -1 unused), set_val (float64
        [Q * max_set], NaN unused) and first_order (float64 [Q]); the re-solved system's answer for
        that set into newton (float64 [Q]) and dtheta (float64 [Q * 3 * D / 2], the extended
        reference theta order); the gap into diff (float64 [Q]).  margin: float64 [Q] >= 0 or None
        (0).  Every output may be None, not all."""
        import torch
        for t, name in ((qu, "qu"), (qi, "qi"), (qj, "qj"), (set_size, "set_size"), (set_row, "set_row")):
            self._need_int32(t, name)
        Q = qu.numel()
        if qi.numel() != Q or qj.numel() != Q:
            raise ValueError("qu, qi and qj must have the same length")
        if isinstance(max_set, bool) or int(max_set) != max_set:
            raise ValueError("max_set must be an integer")
        max_set = int(max_set)
        for t, name in ((margin, "margin"), (set_val, "set_val"), (first_order, "first_order"), (newton, "newton"),
                        (dtheta, "dtheta"), (diff, "diff")):
            if t is not None and t.dtype != torch.float64:
                raise TypeError("%s must be a torch.float64 tensor" % name)
        for t, name in ((qu, "qu"), (qi, "qi"), (qj, "qj"), (margin, "margin"), (set_size, "set_size"),
                        (set_row, "set_row"), (set_val, "set_val"), (first_order, "first_order"),
                        (newton, "newton"), (dtheta, "dtheta"), (diff, "diff")):
            if t is not None and not (t.is_cuda and t.is_contiguous()):
                raise TypeError("%s must be a contiguous device (cuda) tensor" % name)
        # (a max_set out of range is the library's to refuse, before it looks at any array)
        slots = Q * max_set if 1 <= max_set <= FIA_FLIP_MAX_SET else 0
        for t, name, need in ((margin, "margin", Q), (set_size, "set_size", Q), (set_row, "set_row", slots),
                              (set_val, "set_val", slots), (first_order, "first_order", Q), (newton, "newton", Q),
                              (dtheta, "dtheta", Q * (3 * self.num_params() // 2) if dtheta is not None else 0),
                              (diff, "diff", Q)):
            if t is not None and t.numel() < need:
                raise ValueError("%s holds %d values, the batch needs %d" % (name, t.numel(), need))
        rc = self.lib.fia_pair_flip(self.h, Q, _ptr(qu), _ptr(qi), _ptr(qj), _ptr(margin), max_set, _ptr(set_size),
                                    _ptr(set_row), _ptr(set_val), _ptr(first_order), _ptr(newton), _ptr(dtheta),
                                    _ptr(diff), _stream())
        self._check(rc, "fia_pair_flip")

    def count_related_slate(self, qu, slate_offsets, slate_item, offsets=None, want_total=True):
        """fia_count_related_slate: offsets (int64 [Q + 1]) of the slate queries' related lists
        R_u ++ C_i1 ++ .. ++ C_im and, with want_total, their total on the host (then bad ids,
        repeated items, bad slate lengths and entities outside a prepare_for cover raise).  Slate q
        is slate_item[slate_offsets[q] : slate_offsets[q + 1]]."""
        import torch
        for t, name in ((qu, "qu"), (slate_item, "slate_item")):
            self._need_int32(t, name)
        Q = qu.numel()
        if slate_offsets.dtype != torch.int64 or slate_offsets.numel() != Q + 1:
            raise TypeError("slate_offsets must be a torch.int64 tensor of Q + 1 values")
        if not (slate_offsets.is_cuda and slate_offsets.is_contiguous()):
            raise TypeError("slate_offsets must be a contiguous device (cuda) tensor")
        if offsets is None:
            offsets = torch.empty(Q + 1, dtype=torch.int64, device=self.torch_device)
        total = ctypes.c_int64(0)
        rc = self.lib.fia_count_related_slate(self.h, Q, _ptr(qu), _ptr(slate_offsets), slate_item.numel(),
                                              _ptr(slate_item), _ptr(offsets),
                                              ctypes.byref(total) if want_total else None, _stream())
        self._check(rc, "fia_count_related_slate")
        return offsets, (total.value if want_total else None)

    def slate_batch(self, qu, slate_offsets, slate_item, slate_weight, offsets, total, rel_idx=None, influence=None,
                    x=None, value=None, K=0, topk_pos=None, topk_idx=None, topk_val=None):
        """fia_slate_batch: for every slate query (qu; its items; its weights) the influence of every
        rating of R_u ++ C_i1 ++ .. ++ C_im on f = sum_l w_l r-hat(u, i_l) -- one system over
        (theta_u, theta_i1 .. theta_im), solved once -- into influence (float64 [total]), the train
        rows into rel_idx (int32 [total]), x = H^-1 v into x (float64 [Ds * (total_items + Q)], query
        q's at Ds * (slate_offsets[q] + q), the extended reference theta order), f into value
        (float64 [Q]) and, with K, the K ratings of largest |influence| per query (topk_pos /
        topk_idx int64 [Q * K], topk_val float64 [Q * K]).  offsets / total as count_related_slate
        returns them."""
        import torch
        for t, name in ((qu, "qu"), (slate_item, "slate_item"), (rel_idx, "rel_idx")):
            self._need_int32(t, name)
        Q = qu.numel()
        TI = slate_item.numel()
        if slate_weight.numel() != TI:
            raise ValueError("slate_item and slate_weight must have the same length")
        for t, name in ((slate_offsets, "slate_offsets"), (offsets, "offsets")):
            if t.dtype != torch.int64 or t.numel() != Q + 1:
                raise TypeError("%s must be a torch.int64 tensor of Q + 1 values" % name)
        for t, name in ((slate_weight, "slate_weight"), (influence, "influence"), (x, "x"), (value, "value"),
                        (topk_val, "topk_val")):
            if t is not None and t.dtype != torch.float64:
                raise TypeError("%s must be a torch.float64 tensor" % name)
        for t, name in ((topk_pos, "topk_pos"), (topk_idx, "topk_idx")):
            if t is not None and t.dtype != torch.int64:
                raise TypeError("%s must be a torch.int64 tensor" % name)
        for t, name in ((qu, "qu"), (slate_offsets, "slate_offsets"), (slate_item, "slate_item"),
                        (slate_weight, "slate_weight"), (offsets, "offsets"), (rel_idx, "rel_idx"),
                        (influence, "influence"), (x, "x"), (value, "value"), (topk_pos, "topk_pos"),
                        (topk_idx, "topk_idx"), (topk_val, "topk_val")):
            if t is not None and not (t.is_cuda and t.is_contiguous()):
                raise TypeError("%s must be a contiguous device (cuda) tensor" % name)
        # (an oversized total is the library's to refuse, before it looks at any array)
        if 0 <= total < 2 ** 31:
            for t, name in ((rel_idx, "rel_idx"), (influence, "influence")):
                if t is not None and t.numel() < total:
                    raise ValueError("%s holds %d values, the batch has %d related ratings" % (name, t.numel(), total))
        Ds = self.num_params() // 2
        if x is not None and x.numel() < Ds * (TI + Q):
            raise ValueError("x holds %d values, %d queries with %d items need %d" % (x.numel(), Q, TI, Ds * (TI + Q)))
        if value is not None and value.numel() < Q:
            raise ValueError("value holds %d values, the batch has %d queries" % (value.numel(), Q))
        K = int(K)
        if K > 0 and (topk_pos is None or topk_idx is None or topk_val is None
                      or min(topk_pos.numel(), topk_idx.numel(), topk_val.numel()) < Q * K):
            raise ValueError("top-K outputs must hold Q * K values")
        rc = self.lib.fia_slate_batch(self.h, Q, _ptr(qu), _ptr(slate_offsets), TI, _ptr(slate_item),
                                      _ptr(slate_weight), _ptr(offsets), int(total), _ptr(rel_idx), _ptr(influence),
                                      _ptr(x), _ptr(value), K, _ptr(topk_pos), _ptr(topk_idx), _ptr(topk_val),
                                      _stream())
        self._check(rc, "fia_slate_batch")

    # ---- profiling ----
    def set_profiling(self, on, phases=None):
        """on: record HIP-event pairs for the phases named in `phases` (all if None)."""
        mask = 0
        if on:
            mask = 0x1f if phases is None else sum(1 << PHASES.index(p) for p in phases)
        self._set_mask(mask)

    def _set_mask(self, mask):
        self._check(self.lib.fia_set_profiling(self.h, mask), "fia_set_profiling")
        self._mask = mask
        if mask:
            self._pending = True    # events may be recorded until the next drain

    def _drain(self):
        ms = (ctypes.c_double * FIA_NUM_PHASES)()
        cnt = (ctypes.c_int64 * FIA_NUM_PHASES)()
        self._check(self.lib.fia_profile_read(self.h, ms, cnt), "fia_profile_read")
        self._pending = self._mask != 0
        return {PHASES[p]: (ms[p], cnt[p]) for p in range(FIA_NUM_PHASES)}

    def profile_read(self):
        """Per-phase (ms sum, count) recorded since the last read (synchronises the events)."""
        out = self._drain()
        if self._carry is not None:
            out = {p: (out[p][0] + self._carry[p][0], out[p][1] + self._carry[p][1]) for p in PHASES}
            self._carry = None
        return out

    def profiled_call(self, fn):
        """Run fn() with every phase recorded and return (fn's result, its phase sums).  The
        caller's profiling mask and the sums it has accumulated but not yet read are kept
        (the RQ2 timers of a single query, GenericNeuralNet.get_influence_on_test_loss)."""
        # (nothing can be pending when profiling was off since the last drain: skip that read)
        before = self._drain() if getattr(self, "_pending", True) else {p: (0.0, 0) for p in PHASES}
        mask = self._mask
        self._set_mask(0x1f)
        try:
            res = fn()
        finally:
            self._set_mask(mask)
        mine = self._drain()
        if self._carry is not None:
            before = {p: (before[p][0] + self._carry[p][0], before[p][1] + self._carry[p][1]) for p in PHASES}
        self._carry = before
        return res, mine
