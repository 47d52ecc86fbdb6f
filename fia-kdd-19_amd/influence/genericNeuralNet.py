"""Model base of the FIA path: the reference's constructor contract and the
FIA query methods, backed by the HIP library (libfia.so) instead of a
TensorFlow session.

Reference: src/influence/genericNeuralNet.py (GenericNeuralNet.__init__
:82-181) and the per-model FIA methods of matrix_factorization.py:38-67,
152-351 / NCF.py:43-66, 181-380.  Training (gnn:367-449), the classic
full-parameter influence variants (gnn:511-808) and TF checkpoints are not
part of this build.

Training and leave-one-out retraining (gnn:344-412) run
on influence/train.py (PyTorch-ROCm, TF-Adam); checkpoints are npz files with
the parameters and the Adam state (the TF Saver keeps both, gnn:149, 410).
"""
import os
import time

import numpy as np

from influence import _lib
from influence.dataset import DataSet


def rq2_timing(phases, n, wall_s, log=None):
    """The reference's three RQ2 stage timers (mf:224-250: 'Inverse HVP took', 'Multiplying by
    n train examples took', 'Total time is') from the library's per-phase HIP-event sums
    (ms, count) of one query call: the inverse HVP is the related-list build ('chunks'), the
    per-entity Hessian caches if rebuilt ('prepare') and the exact solve ('solve'); the
    multiplication is the per-rating scoring ('score') and the top-K merge ('topk').
    Returns dict(inverse_hvp_s, multiply_s, total_s, wall_s, n)."""
    ms = {p: float(v[0]) for p, v in phases.items()}
    inv = (ms.get("chunks", 0.0) + ms.get("prepare", 0.0) + ms.get("solve", 0.0)) * 1e-3
    mul = (ms.get("score", 0.0) + ms.get("topk", 0.0)) * 1e-3
    t = dict(inverse_hvp_s=inv, multiply_s=mul, total_s=inv + mul, wall_s=float(wall_s), n=int(n))
    if log is not None:
        log("Inverse HVP took %s sec" % inv)
        log("Multiplying by %s train examples took %s sec" % (n, mul))
        log("Total time is %s sec" % (inv + mul))
    return t


class GenericNeuralNet(object):
    MODEL_ID = None          # _lib.FIA_MODEL_MF / _lib.FIA_MODEL_NCF
    PARAM_NAMES = ()         # reference variable names, include/fia.h table order

    def __init__(self, **kwargs):
        np.random.seed(0)    # gnn:83 -- RQ1's query choice (RQ1.py:132) depends on it
        self.batch_size = kwargs.pop("batch_size")
        self.data_sets = kwargs.pop("data_sets")
        self.train_dir = kwargs.pop("train_dir", "output")
        self.log_dir = kwargs.pop("log_dir", "log")
        self.model_name = kwargs.pop("model_name")
        self.num_classes = kwargs.pop("num_classes")
        self.initial_learning_rate = kwargs.pop("initial_learning_rate")
        self.decay_epochs = kwargs.pop("decay_epochs")
        self.avextol = kwargs.pop("avextol")
        self.keep_probs = kwargs.pop("keep_probs", None)
        self.mini_batch = kwargs.pop("mini_batch", True)
        self.damping = kwargs.pop("damping", 0.0)
        self.device = kwargs.pop("device", 0)
        self.verbose = kwargs.pop("verbose", True)
        self.save_inverse_hvp = kwargs.pop("save_inverse_hvp", True)
        params = kwargs.pop("params", None)
        if not os.path.exists(self.train_dir):
            os.makedirs(self.train_dir)
        train = self.data_sets["train"]
        self.num_train_examples = train.labels.shape[0]
        self.num_test_examples = self.data_sets["test"].labels.shape[0]
        self.ctx = _lib.Context(self.device)
        self.params = self.init_params(seed=0) if params is None else self._checked(params)
        self._upload_params()
        self._build_index(train)
        self.ctx.prepare()

    # ------------------------------------------------------------------ params
    def param_shapes(self):
        raise NotImplementedError

    def init_params(self, seed=0):
        raise NotImplementedError

    def _checked(self, params):
        shapes = self.param_shapes()
        out = {}
        for name in self.PARAM_NAMES:
            if name not in params:
                raise ValueError("missing parameter %s" % name)
            a = np.ascontiguousarray(np.asarray(params[name], np.float32).reshape(-1))
            if a.shape != shapes[name]:
                raise ValueError("parameter %s has shape %s, expected %s" % (name, a.shape, shapes[name]))
            out[name] = a
        return out

    def _upload_params(self):
        import torch
        self._dev_params = [torch.from_numpy(self.params[n]).to(self.ctx.torch_device) for n in self.PARAM_NAMES]
        self.ctx.set_params(self.MODEL_ID, self.embedding_size, self.num_users, self.num_items, self._dev_params,
                            self.weight_decay, self.damping)

    def load_params(self, params):
        """Replace the parameter values (e.g. trained elsewhere) and rebuild the Hessian caches."""
        self.params = self._checked(params)
        self._upload_params()
        self.ctx.prepare()

    def prepare_for(self, test_indices, other_items=None):
        """Rebuild the Hessian caches for only the users/items of these test ratings
        (fia_prepare_for: one GPU's share of a sharded query set at large k).  Queries
        outside the set then raise FIAError until the next prepare.  other_items (optional,
        one item per test rating): also cover the pairs (u_t, other_items[t]), the j's of a
        shard's get_pair_influence_batch calls."""
        oj = None if other_items is None else self._checked_other_items(test_indices, other_items)
        qu, qi = self._query_tensors(test_indices)
        if oj is not None:
            import torch
            qu, qi = torch.cat([qu, qu]), torch.cat([qi, torch.from_numpy(oj).to(self.ctx.torch_device)])
        self.ctx.prepare_for(qu, qi)

    def get_all_params(self):
        """Parameter values in the reference's get_all_params order (mf:30-36)."""
        return [self.params[n] for n in self.PARAM_NAMES]

    @property
    def checkpoint_file(self):
        return os.path.join(self.train_dir, "%s-checkpoint" % self.model_name)   # gnn:169

    def save_checkpoint(self, step):
        """npz checkpoint: parameters (reference names) + the trainer's Adam state."""
        path = "%s-%s.npz" % (self.checkpoint_file, step)
        arrs = {n.replace("/", "__"): v for n, v in self.params.items()}
        tr = getattr(self, "_tr", None)
        if tr is not None:
            st = tr.opt.state()
            for j, n in enumerate(self.PARAM_NAMES):
                arrs["adam_m__" + n.replace("/", "__")] = st["m"][j]
                arrs["adam_v__" + n.replace("/", "__")] = st["v"][j]
            arrs["adam_b1p"] = np.float32(st["b1p"])
            arrs["adam_b2p"] = np.float32(st["b2p"])
        np.savez(path, **arrs)
        return path

    def load_checkpoint(self, iter_to_load, do_checks=True):
        """npz checkpoints written by save_checkpoint (saver.restore, gnn:414-420).  TF
        checkpoints of the reference are read by influence.tf_checkpoint."""
        path = "%s-%s.npz" % (self.checkpoint_file, iter_to_load)
        with np.load(path, allow_pickle=False) as z:
            files = set(z.files)
            self.load_params({n: z[n.replace("/", "__")] for n in self.PARAM_NAMES})
            tr = getattr(self, "_tr", None)
            if tr is not None:
                tr.set_params(self.params)
                if "adam_b1p" in files:
                    tr.opt.load_state({"m": [z["adam_m__" + n.replace("/", "__")] for n in self.PARAM_NAMES],
                                       "v": [z["adam_v__" + n.replace("/", "__")] for n in self.PARAM_NAMES],
                                       "b1p": float(z["adam_b1p"]), "b2p": float(z["adam_b2p"])})
                else:
                    tr.opt.reset()
        if self.verbose:
            print("Loading successful...")

    def load_tf_checkpoint(self, prefix):
        """Load a reference TF checkpoint-V2 bundle (tf.train.Saver output, e.g.
        output/<model_name>-checkpoint-<step>) without TensorFlow: the variables under the
        reference names, plus the Adam slots <var>/Adam, <var>/Adam_1 and beta powers when
        present (influence/tf_checkpoint.py)."""
        from influence import tf_checkpoint as tfc
        t = tfc.read_checkpoint(prefix)
        missing = [n for n in self.PARAM_NAMES if n not in t]
        if missing:
            raise ValueError("checkpoint %s lacks %s" % (prefix, ", ".join(missing)))
        self.load_params({n: t[n].reshape(-1) for n in self.PARAM_NAMES})
        tr = getattr(self, "_tr", None)
        if tr is not None:
            tr.set_params(self.params)
            slots = all(n + "/Adam" in t and n + "/Adam_1" in t for n in self.PARAM_NAMES)
            if slots and "beta1_power" in t and "beta2_power" in t:
                tr.opt.load_state({"m": [t[n + "/Adam"].reshape(-1) for n in self.PARAM_NAMES],
                                   "v": [t[n + "/Adam_1"].reshape(-1) for n in self.PARAM_NAMES],
                                   "b1p": float(t["beta1_power"]), "b2p": float(t["beta2_power"])})
            else:
                tr.opt.reset()

    def save_tf_checkpoint(self, prefix):
        """Write the parameters (and the trainer's Adam state) as a TF checkpoint-V2 bundle
        under the reference variable names."""
        from influence import tf_checkpoint as tfc
        t = {n: np.asarray(self.params[n], np.float32) for n in self.PARAM_NAMES}
        tr = getattr(self, "_tr", None)
        if tr is not None:
            st = tr.opt.state()
            for j, n in enumerate(self.PARAM_NAMES):
                t[n + "/Adam"] = st["m"][j]
                t[n + "/Adam_1"] = st["v"][j]
            t["beta1_power"] = np.float32(st["b1p"])
            t["beta2_power"] = np.float32(st["b2p"])
        tfc.write_checkpoint(prefix, t)
        return prefix

    # ---------------------------------------------------------------- training
    @property
    def model_kind(self):
        return "MF" if self.MODEL_ID == _lib.FIA_MODEL_MF else "NCF"

    def trainer(self):
        """The model's TF-Adam trainer (created on first use from the current params)."""
        if getattr(self, "_tr", None) is None:
            from influence.train import Trainer
            self._tr = Trainer(self.model_kind, self.embedding_size, self.weight_decay, self.initial_learning_rate,
                               self.params, self.PARAM_NAMES, self.ctx.torch_device)
        return self._tr

    def _sync_from_trainer(self):
        """Trained values -> FIA context (re-upload + Hessian caches)."""
        self.load_params(self.trainer().params_numpy())

    def train(self, num_steps, iter_to_switch_to_batch=10000000, iter_to_switch_to_sgd=10000000,
              save_checkpoints=True, verbose=True, load_checkpoints=False):
        """Adam on reference mini-batches (gnn:367-412): steps load_checkpoints+1 .. num_steps-1,
        then the parameters go to the FIA context and, with save_checkpoints, a checkpoint
        num_steps-1 is written (the reference saves only past step 20000; this build always
        saves at the end).  The SGD phase (gnn:395-397) is not used by the reference scripts
        and is not provided."""
        if iter_to_switch_to_sgd < num_steps:
            raise NotImplementedError("the SGD phase of GenericNeuralNet.train is not provided")
        tr = self.trainer()
        if load_checkpoints:
            self.load_checkpoint(load_checkpoints, do_checks=False)
        else:
            load_checkpoints = 0
        train = self.data_sets["train"]
        full = None
        ran = False
        for step in range(load_checkpoints + 1, num_steps):
            t0 = time.time()
            if step < iter_to_switch_to_batch:
                xb, yb = train.next_batch(self.batch_size)
                loss = tr.step(xb[:, 0].astype(np.int64), xb[:, 1].astype(np.int64), yb)
            else:
                if full is None:
                    full = self.fill_feed_dict_with_all_ex(train)
                loss = tr.step(full["users"], full["items"], full["labels"])
            ran = True
            if verbose and step % 1000 == 0:
                print("Step %d: loss = %.8f (%.3f sec)" % (step, float(loss), time.time() - t0))
        if ran:
            self._sync_from_trainer()
            if save_checkpoints:
                self.save_checkpoint(num_steps - 1)

    def fill_feed_dict_with_all_ex(self, data_set):
        """All rows (gnn:210-215), as index arrays for the trainer."""
        x = np.asarray(data_set.x)
        return {"users": x[:, 0].astype(np.int64), "items": x[:, 1].astype(np.int64),
                "labels": np.asarray(data_set.labels, np.float32)}

    def fill_feed_dict_with_all_but_one_ex(self, data_set, idx_to_remove):
        """All rows but train row idx_to_remove (gnn:218-227)."""
        keep = np.ones(data_set.x.shape[0], bool)
        keep[idx_to_remove] = False
        x = np.asarray(data_set.x)[keep]
        return {"users": x[:, 0].astype(np.int64), "items": x[:, 1].astype(np.int64),
                "labels": np.asarray(data_set.labels, np.float32)[keep]}

    def retrain(self, num_steps, feed_dict):
        """GenericNeuralNet.retrain (gnn:344-347): num_steps Adam steps on ALL of feed_dict's
        rows at once.  MF and NCF override it with the reference's mini-batch retrain
        (mf:69-76, NCF.py:68-72); this full-batch form stays available to them as
        retrain_full_batch."""
        self.retrain_full_batch(num_steps, feed_dict)

    def retrain_full_batch(self, num_steps, feed_dict):
        """num_steps full-batch Adam steps on feed_dict's rows, one HIP graph replay per step
        (opt-in fast path; not the MF / NCF reference procedure).  Only the trainer's
        parameters change (the FIA context keeps the loaded model)."""
        self.trainer().full_batch(feed_dict["users"], feed_dict["items"], feed_dict["labels"], num_steps)

    def _retrain_minibatch(self, num_steps, feed_dict):
        """The MF / NCF retrain body: DataSet(feed rows) + num_steps steps on
        next_batch(self.batch_size) (fill_feed_dict_with_batch, gnn:229-240)."""
        x = np.stack([np.asarray(feed_dict["users"]), np.asarray(feed_dict["items"])], 1)
        ds = DataSet(x, np.asarray(feed_dict["labels"]))
        tr = self.trainer()
        for _ in range(num_steps):
            xb, yb = ds.next_batch(self.batch_size)
            tr.step(xb[:, 0].astype(np.int64), xb[:, 1].astype(np.int64), yb)

    def reset_optimizer(self):
        """reset_optimizer_op (gnn:437-438)."""
        self.trainer().opt.reset()

    def predict_pairs(self, users, items):
        """Trainer-side r-hat (float64) for (user, item) pairs."""
        return self.trainer().predict(np.asarray(users, np.int64), np.asarray(items, np.int64))

    def predict_test(self, test_idx):
        """r-hat of test rating test_idx under the trainer's current parameters (model.logits)."""
        u, i = self._test_pair(test_idx)
        return float(self.predict_pairs([u], [i])[0])

    def train_loss(self):
        """total_loss on all training rows under the trainer's parameters."""
        f = self.fill_feed_dict_with_all_ex(self.data_sets["train"])
        return self.trainer().loss(f["users"], f["items"], f["labels"])

    # ------------------------------------------------------------------- index
    def _build_index(self, train):
        import torch
        x = np.asarray(train.x)
        users = getattr(train, "users", None)
        items = getattr(train, "items", None)
        if users is None:
            users = x[:, 0].astype(np.int32)
            items = x[:, 1].astype(np.int32)
        dev = self.ctx.torch_device
        self._train_users = torch.from_numpy(np.ascontiguousarray(users, np.int32)).to(dev)
        self._train_items = torch.from_numpy(np.ascontiguousarray(items, np.int32)).to(dev)
        self._train_ratings = torch.from_numpy(np.ascontiguousarray(train.labels, np.float32)).to(dev)
        self.ctx.build_index(self._train_users, self._train_items, self._train_ratings, self.num_users,
                             self.num_items)
        # host degree counts: a single query's related-set size without a count round trip
        self._deg_u = np.bincount(np.asarray(users, np.int64), minlength=self.num_users)
        self._deg_i = np.bincount(np.asarray(items, np.int64), minlength=self.num_items)

    # --------------------------------------------------------------- queries
    def _test_pair(self, test_index):
        test_u, test_i = self.data_sets["test"].x[test_index]
        return int(test_u), int(test_i)

    def _query_tensors(self, test_indices):
        import torch
        pairs = np.array([self._test_pair(t) for t in test_indices], np.int32).reshape(-1, 2)
        dev = self.ctx.torch_device
        qu = torch.from_numpy(np.ascontiguousarray(pairs[:, 0])).to(dev)
        qi = torch.from_numpy(np.ascontiguousarray(pairs[:, 1])).to(dev)
        return qu, qi

    def get_train_indices_of_test_case(self, test_indices):
        """rel = where(train.x[:,0]==u) ++ where(train.x[:,1]==i) (mf:315-322), from the GPU index."""
        import torch
        assert len(test_indices) == 1
        self.test_u, self.test_i = self._test_pair(test_indices[0])
        qu, qi = self._query_tensors(test_indices)
        offsets, total = self.ctx.count_related(qu, qi)
        rel = torch.empty(max(total, 1), dtype=torch.int32, device=self.ctx.torch_device)
        self.ctx.related(qu, qi, offsets, rel)
        return rel[:total].cpu().numpy().astype(np.int64)     # the reference's np.where dtype

    def get_test_params(self, test_index):
        """theta_t values in the reference block order (mf:38-67 / ncf:43-66)."""
        u, i = self._test_pair(test_index[0])
        return self._theta_blocks(u, i)

    def get_influence_batch(self, test_indices, K=1, full=True, return_x=True, inverse_hvp=None):
        """Batched FIA over many test ratings (one fia_query_batch call).

        inverse_hvp (optional, float64 [Q, D] in the reference theta order): score with these
        inverse HVPs instead of solving (fia_query_batch_x; returned as x).
        Returns dict(offsets, rel_idx, influence, x, topk_pos, topk_idx, topk_val) as numpy
        arrays; influence[offsets[q]:offsets[q+1]] is get_influence_on_test_loss([t_q], ...)."""
        import torch
        qu, qi = self._query_tensors(test_indices)
        Q = qu.numel()
        dev = self.ctx.torch_device
        offsets, total = self.ctx.count_related(qu, qi)
        D = self.ctx.num_params()
        rel = torch.empty(max(total, 1), dtype=torch.int32, device=dev) if full else None
        infl = torch.empty(max(total, 1), dtype=torch.float64, device=dev) if full else None
        tp = torch.empty(max(Q * K, 1), dtype=torch.int64, device=dev) if K else None
        ti = torch.empty(max(Q * K, 1), dtype=torch.int64, device=dev) if K else None
        tv = torch.empty(max(Q * K, 1), dtype=torch.float64, device=dev) if K else None
        if inverse_hvp is not None:
            xin = np.ascontiguousarray(np.asarray(inverse_hvp, np.float64).reshape(-1))
            if xin.size != Q * D:
                raise ValueError("inverse_hvp must hold %d x %d values" % (Q, D))
            x = torch.from_numpy(xin).to(dev)
            self.ctx.query_batch_x(qu, qi, offsets, total, x, rel, infl, K, tp, ti, tv)
        else:
            x = torch.empty(max(Q * D, 1), dtype=torch.float64, device=dev) if return_x else None
            self.ctx.query_batch(qu, qi, offsets, total, rel, infl, x, K, tp, ti, tv)
        out = dict(offsets=offsets.cpu().numpy())
        if full:
            out["rel_idx"] = rel[:total].cpu().numpy().astype(np.int64)
            out["influence"] = infl[:total].cpu().numpy()
        if return_x:
            out["x"] = x[:Q * D].cpu().numpy().reshape(Q, D)
        if K:
            out["topk_pos"] = tp[:Q * K].cpu().numpy().reshape(Q, K)
            out["topk_idx"] = ti[:Q * K].cpu().numpy().reshape(Q, K)
            out["topk_val"] = tv[:Q * K].cpu().numpy().reshape(Q, K)
        return out

    def _checked_candidates(self, n_queries, cand_offsets, X, Y):
        """Host validation of a candidate batch (no GPU call): returns (offsets int64[Q+1],
        users int32[M], items int32[M], ratings float32[M]) or raises ValueError."""
        off = np.asarray(cand_offsets)
        if off.ndim != 1 or off.size != n_queries + 1 or off.dtype.kind not in "iu":
            raise ValueError("cand_offsets must be an integer array of len(test_indices) + 1 values")
        off = np.ascontiguousarray(off, np.int64)
        X = np.asarray(X)
        Y = np.asarray(Y)
        if X.ndim != 2 or X.shape[1] != 2:
            raise ValueError("X must have shape [M, 2] (user, item)")
        if Y.ndim != 1 or Y.shape[0] != X.shape[0]:
            raise ValueError("X and Y must have the same length.")
        m = X.shape[0]
        if off[0] != 0 or off[-1] != m or (np.diff(off) < 0).any():
            raise ValueError("cand_offsets must start at 0, never decrease and end at len(Y) = %d" % m)
        if m and X.dtype.kind == "f" and not (np.isfinite(X).all() and (X == np.floor(X)).all()):
            raise ValueError("candidate ids must be integers")
        users = X[:, 0].astype(np.int64)
        items = X[:, 1].astype(np.int64)
        if m and (users.min() < 0 or users.max() >= self.num_users or items.min() < 0 or
                  items.max() >= self.num_items):
            raise ValueError("candidate ids must lie in [0, %d) x [0, %d)" % (self.num_users, self.num_items))
        return (off, np.ascontiguousarray(users, np.int32), np.ascontiguousarray(items, np.int32),
                np.ascontiguousarray(Y, np.float32))

    def get_candidate_influence_batch(self, test_indices, cand_offsets, X, Y, K=0, full=True, inverse_hvp=None):
        """Influence of HYPOTHETICAL ratings on the predictions of many test ratings (one
        fia_score_candidates call): candidates cand_offsets[q]:cand_offsets[q+1] -- rows of
        X [M, 2] (user, item) with ratings Y [M] -- belong to test rating test_indices[q].  A
        candidate need not be a train row and need not share the query's user or item:

            influence_c = x_q . (2 (r-hat(a, b) - y) d r-hat(a, b)/d theta_t + wd M theta_t) / n_q

        with n_q the query's related-set size, so a candidate equal to a related train row gets
        that row's influence (include/fia.h).  x_q comes from one fia_query_batch call (no
        per-rating vectors), or from inverse_hvp (float64 [Q, D], reference theta order) as in
        get_influence_batch.  Shapes, offsets and id ranges are checked on the host (ValueError)
        before any GPU call.  Returns dict(cand_offsets, influence, x, topk_pos, topk_val) as
        numpy arrays (influence only with full, top-K only with K: positions inside each query's
        candidate list, -1 / NaN where the list is shorter than K)."""
        off, cu, ci, cy = self._checked_candidates(len(test_indices), cand_offsets, X, Y)
        if not 0 <= int(K) <= _lib.FIA_MAX_TOPK:
            raise ValueError("K must be in [0, %d]" % _lib.FIA_MAX_TOPK)
        import torch
        K = int(K)
        qu, qi = self._query_tensors(test_indices)
        Q = qu.numel()
        dev = self.ctx.torch_device
        D = self.ctx.num_params()
        # (the count also rejects query ids out of range and queries outside a prepare_for cover)
        offsets, total = self.ctx.count_related(qu, qi)
        if inverse_hvp is not None:
            xin = np.ascontiguousarray(np.asarray(inverse_hvp, np.float64).reshape(-1))
            if xin.size != Q * D:
                raise ValueError("inverse_hvp must hold %d x %d values" % (Q, D))
            x = torch.from_numpy(xin).to(dev)
        else:
            x = torch.empty(max(Q * D, 1), dtype=torch.float64, device=dev)
            self.ctx.query_batch(qu, qi, offsets, total, None, None, x, 0, None, None, None)
        m = cy.size
        d_off = torch.from_numpy(off).to(dev)
        d_cu = torch.from_numpy(cu).to(dev) if m else torch.empty(1, dtype=torch.int32, device=dev)
        d_ci = torch.from_numpy(ci).to(dev) if m else torch.empty(1, dtype=torch.int32, device=dev)
        d_cy = torch.from_numpy(cy).to(dev) if m else torch.empty(1, dtype=torch.float32, device=dev)
        infl = torch.empty(max(m, 1), dtype=torch.float64, device=dev) if full else None
        tp = torch.empty(max(Q * K, 1), dtype=torch.int64, device=dev) if K else None
        tv = torch.empty(max(Q * K, 1), dtype=torch.float64, device=dev) if K else None
        self.ctx.score_candidates(qu, qi, x, d_off, m, d_cu, d_ci, d_cy, infl, K, tp, tv)
        out = dict(cand_offsets=off, x=x[:Q * D].cpu().numpy().reshape(Q, D))
        if full:
            out["influence"] = infl[:m].cpu().numpy()
        if K:
            out["topk_pos"] = tp[:Q * K].cpu().numpy().reshape(Q, K)
            out["topk_val"] = tv[:Q * K].cpu().numpy().reshape(Q, K)
        return out

    def get_candidate_newton_batch(self, test_indices, cand_offsets, X, Y, K=0, full=True):
        """Newton-corrected influence of HYPOTHETICAL ratings on the predictions of many test
        ratings (one fia_score_candidates_newton call): get_candidate_influence_batch with the
        candidate's own curvature in the system,

            newton_c = v . (H + H_c)^-1 b_c,   H_c = (2 g_c g_c^T + 2 e_c C [a == u and b == i] + wd diag(M)) / n_q,
                                               b_c = (2 e_c g_c + wd M theta_t) / n_q

        (include/fia.h) -- one Newton step of the objective with the rating added; the predicted
        change of r-hat(u, i) is -newton_c.  Candidates cand_offsets[q]:cand_offsets[q+1] -- rows of
        X [M, 2] (user, item) with ratings Y [M] -- belong to test rating test_indices[q].  There is
        no inverse_hvp: the call factorises each query's system itself.  Shapes, offsets, id ranges
        and K (an integer in [0, FIA_MAX_TOPK]; full=False needs K > 0) are checked on the host
        (ValueError) before any GPU call.  Returns dict(cand_offsets, newton, topk_pos, topk_val) as
        numpy arrays (newton only with full, top-K only with K: positions inside each query's
        candidate list, -1 / NaN where the list is shorter than K).  The large-k models raise
        FIAError (unsupported)."""
        off, cu, ci, cy = self._checked_candidates(len(test_indices), cand_offsets, X, Y)
        if isinstance(K, bool) or int(K) != K or not 0 <= int(K) <= _lib.FIA_MAX_TOPK:
            raise ValueError("K must be in [0, %d]" % _lib.FIA_MAX_TOPK)
        K = int(K)
        if not full and K == 0:
            raise ValueError("nothing to return: full=False needs K > 0")
        import torch
        qu, qi = self._query_tensors(test_indices)
        Q = qu.numel()
        dev = self.ctx.torch_device
        # (the count rejects query ids out of range and queries outside a prepare_for cover)
        self.ctx.count_related(qu, qi)
        m = cy.size
        d_off = torch.from_numpy(off).to(dev)
        d_cu = torch.from_numpy(cu).to(dev) if m else torch.empty(1, dtype=torch.int32, device=dev)
        d_ci = torch.from_numpy(ci).to(dev) if m else torch.empty(1, dtype=torch.int32, device=dev)
        d_cy = torch.from_numpy(cy).to(dev) if m else torch.empty(1, dtype=torch.float32, device=dev)
        nw = torch.empty(max(m, 1), dtype=torch.float64, device=dev) if full else None
        tp = torch.empty(max(Q * K, 1), dtype=torch.int64, device=dev) if K else None
        tv = torch.empty(max(Q * K, 1), dtype=torch.float64, device=dev) if K else None
        self.ctx.score_candidates_newton(qu, qi, d_off, m, d_cu, d_ci, d_cy, nw, K, tp, tv)
        out = dict(cand_offsets=off)
        if full:
            out["newton"] = nw[:m].cpu().numpy()
        if K:
            out["topk_pos"] = tp[:Q * K].cpu().numpy().reshape(Q, K)
            out["topk_val"] = tv[:Q * K].cpu().numpy().reshape(Q, K)
        return out

    def _host_num_params(self):
        """D of theta_t from the model's shape alone (no GPU context needed)."""
        k = int(self.embedding_size)
        return 2 * k + 2 if self.MODEL_ID == _lib.FIA_MODEL_MF else 4 * k

    def get_total_influence(self, test_indices, weights=None, K=0, full=True, inverse_hvp=None):
        """Influence of EVERY training rating on a set of predictions (one fia_total_influence
        call; the reference asserts len(test_indices) == 1, matrix_factorization.py:179):

            total[j] = sum_q weights[q] * (influence of train row j on test rating test_indices[q])

        summed over both occurrences when row j is the test pair itself -- the scatter-add by
        rel_idx of get_influence_batch's influence, computed from per-user / per-item sums of the
        queries without walking the related lists (include/fia.h).  count[j] is how often row j
        occurs in the related lists of the batch.  x_q comes from one fia_query_batch call (no
        per-rating vectors), or from inverse_hvp (float64 [Q, D], reference theta order); with
        weights (float [Q], finite) x_q is scaled by weights[q] on the device.  A test rating
        with an empty related set contributes nothing.  weights, K and the inverse_hvp size are
        checked on the host (ValueError) before any GPU call.  Returns dict(x [Q, D] unscaled,
        total float64 [n_train] and count int32 [n_train] with full, topk_idx int64 [K] and
        topk_val float64 [K] with K: the train rows of largest |total| among the touched rows,
        ties to the lower row, -1 / NaN where fewer than K rows are touched)."""
        Q = len(test_indices)
        D = self._host_num_params()
        w = None
        if weights is not None:
            w = np.asarray(weights, np.float64)
            if w.ndim != 1 or w.size != Q:
                raise ValueError("weights must hold len(test_indices) = %d values" % Q)
            if not np.isfinite(w).all():
                raise ValueError("weights must be finite")
        if int(K) != K or not 0 <= int(K) <= _lib.FIA_MAX_TOPK:
            raise ValueError("K must be in [0, %d]" % _lib.FIA_MAX_TOPK)
        K = int(K)
        xin = None
        if inverse_hvp is not None:
            xin = np.ascontiguousarray(np.asarray(inverse_hvp, np.float64).reshape(-1))
            if xin.size != Q * D:
                raise ValueError("inverse_hvp must hold %d x %d values" % (Q, D))
        if not full and K == 0:
            raise ValueError("nothing to return: full=False needs K > 0")
        import torch
        qu, qi = self._query_tensors(test_indices)
        dev = self.ctx.torch_device
        if xin is not None:
            x = torch.from_numpy(xin).to(dev) if Q else torch.empty(1, dtype=torch.float64, device=dev)
        else:
            # (the count also rejects query ids out of range and queries outside a prepare_for cover)
            offsets, total_rel = self.ctx.count_related(qu, qi)
            x = torch.empty(max(Q * D, 1), dtype=torch.float64, device=dev)
            self.ctx.query_batch(qu, qi, offsets, total_rel, None, None, x, 0, None, None, None)
        xs = x
        if w is not None and Q:
            xs = (x[:Q * D].view(Q, D) * torch.from_numpy(w).to(dev)[:, None]).reshape(-1).contiguous()
        n = self.ctx.n_train
        total = torch.empty(max(n, 1), dtype=torch.float64, device=dev) if full else None
        count = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if full else None
        ti = torch.empty(max(K, 1), dtype=torch.int64, device=dev) if K else None
        tv = torch.empty(max(K, 1), dtype=torch.float64, device=dev) if K else None
        self.ctx.total_influence(qu, qi, xs, total, count, K, ti, tv)
        out = dict(x=x[:Q * D].cpu().numpy().reshape(Q, D))
        if full:
            out["total"] = total[:n].cpu().numpy()
            out["count"] = count[:n].cpu().numpy()
        if K:
            out["topk_idx"] = ti[:K].cpu().numpy()
            out["topk_val"] = tv[:K].cpu().numpy()
        return out

    def _checked_groups(self, n_queries, groups):
        """Host validation of get_group_influence's groups (no GPU call): returns (grp_offsets
        int64 [Q+1], mem_offsets int64 [G+1], mem_row int32 [total]) or raises ValueError."""
        if len(groups) != n_queries:
            raise ValueError("groups must hold one sequence of groups per test index (%d, got %d)" % (
                n_queries, len(groups)))
        n_train = int(self.num_train_examples)
        grp_off, mem_off, rows = [0], [0], []
        for per_query in groups:
            for grp in per_query:
                r = np.asarray(grp)
                if r.size == 0:
                    r = np.zeros(0, np.int64)
                if r.ndim != 1:
                    raise ValueError("a group must be a 1-d array of train rows")
                if r.dtype.kind not in "iu":
                    raise ValueError("train rows must be integers (got dtype %s)" % r.dtype)
                r = r.astype(np.int64)
                if r.size and (r.min() < 0 or r.max() >= n_train):
                    raise ValueError("train rows must lie in [0, %d)" % n_train)
                if np.unique(r).size != r.size:
                    raise ValueError("a group lists a train row more than once")
                rows.append(r)
                mem_off.append(mem_off[-1] + r.size)
            grp_off.append(len(mem_off) - 1)
        mem_row = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        return (np.asarray(grp_off, np.int64), np.asarray(mem_off, np.int64),
                np.ascontiguousarray(mem_row, np.int32))

    def get_group_influence(self, test_indices, groups, return_dtheta=False, inverse_hvp=None):
        """Effect of removing SETS of training ratings on the predictions of test ratings (one
        fia_group_influence call; the reference scores one rating at a time).  groups[q] is a
        sequence of integer arrays of train rows, the groups of test rating test_indices[q]; it
        may be empty, and so may a group.  For each group S

            group       = v . (H - H_S)^-1 b_S      the system without S's ratings, solved again
            first_order = (H^-1 v) . b_S            the sum of S's single-rating influences

        (include/fia.h).  Sign convention: that of get_influence_on_test_loss -- the predicted
        change of r-hat(u, i) when the ratings are removed.  A row that shares neither the test
        rating's user nor its item contributes nothing; the test pair's own train row counts
        twice, as in its related list.  inverse_hvp (float64 [Q, D], reference theta order), when
        given, is only checked for its size: first_order always comes from the exact solve.
        len(groups), integer rows, their range and duplicates inside a group are checked on the
        host (ValueError) before any GPU call.  Returns dict(grp_offsets int64 [Q+1], mem_offsets
        int64 [G+1], group float64 [G], first_order float64 [G], and with return_dtheta dtheta
        float64 [G, D], the parameter step in the reference theta order) as numpy arrays."""
        Q = len(test_indices)
        grp_off, mem_off, mem_row = self._checked_groups(Q, groups)
        D = self._host_num_params()
        if inverse_hvp is not None and np.asarray(inverse_hvp).size != Q * D:
            raise ValueError("inverse_hvp must hold %d x %d values" % (Q, D))
        import torch
        G = mem_off.size - 1
        qu, qi = self._query_tensors(test_indices)
        dev = self.ctx.torch_device
        # (the count rejects query ids out of range and queries outside a prepare_for cover)
        self.ctx.count_related(qu, qi)
        d_go = torch.from_numpy(grp_off).to(dev)
        d_mo = torch.from_numpy(mem_off).to(dev)
        d_mr = torch.from_numpy(mem_row).to(dev) if mem_row.size else torch.empty(1, dtype=torch.int32, device=dev)[:0]
        grp = torch.empty(max(G, 1), dtype=torch.float64, device=dev)
        fo = torch.empty(max(G, 1), dtype=torch.float64, device=dev)
        dth = torch.empty(max(G * D, 1), dtype=torch.float64, device=dev) if return_dtheta else None
        self.ctx.group_influence(qu, qi, d_go, d_mo, d_mr, grp, fo, dth)
        out = dict(grp_offsets=grp_off, mem_offsets=mem_off, group=grp[:G].cpu().numpy(),
                   first_order=fo[:G].cpu().numpy())
        if return_dtheta:
            out["dtheta"] = dth[:G * D].cpu().numpy().reshape(G, D)
        return out

    def _checked_edits(self, n_queries, edits):
        """Host validation of get_edit_influence's edit sets (no GPU call): returns (grp_offsets
        int64 [Q+1], rem_offsets int64 [G+1], rem_row int32, add_offsets int64 [G+1], add_user,
        add_item int32, add_rating float32) or raises ValueError."""
        if len(edits) != n_queries:
            raise ValueError("edits must hold one sequence of groups per test index (%d, got %d)" % (
                n_queries, len(edits)))
        n_train = int(self.num_train_examples)
        grp_off, rem_off, add_off, rows, adds = [0], [0], [0], [], []
        for per_query in edits:
            for grp in per_query:
                if isinstance(grp, np.ndarray) or not hasattr(grp, "__len__") or len(grp) != 2:
                    raise ValueError("a group must be a pair (remove_rows, add_triples)")
                r = np.asarray(grp[0])
                if r.size == 0:
                    r = np.zeros(0, np.int64)
                if r.ndim != 1:
                    raise ValueError("remove_rows must be a 1-d array of train rows")
                if r.dtype.kind not in "iu":
                    raise ValueError("train rows must be integers (got dtype %s)" % r.dtype)
                r = r.astype(np.int64)
                if r.size and (r.min() < 0 or r.max() >= n_train):
                    raise ValueError("train rows must lie in [0, %d)" % n_train)
                if np.unique(r).size != r.size:
                    raise ValueError("a group removes a train row more than once")
                try:
                    a = np.asarray(grp[1], np.float64)
                except (TypeError, ValueError):
                    raise ValueError("add_triples must be an array-like of (user, item, rating)")
                if a.size == 0:
                    a = np.zeros((0, 3))
                if a.ndim != 2 or a.shape[1] != 3:
                    raise ValueError("add_triples must have shape [m, 3]: (user, item, rating)")
                if not np.isfinite(a).all():
                    raise ValueError("added ids and ratings must be finite")
                if (a[:, :2] != np.floor(a[:, :2])).any():
                    raise ValueError("added ids must be integers")
                if a.shape[0] and (a[:, 0].min() < 0 or a[:, 0].max() >= self.num_users or a[:, 1].min() < 0 or
                                   a[:, 1].max() >= self.num_items):
                    raise ValueError("added ids must lie in [0, %d) x [0, %d)" % (self.num_users, self.num_items))
                rows.append(r)
                adds.append(a)
                rem_off.append(rem_off[-1] + r.size)
                add_off.append(add_off[-1] + a.shape[0])
            grp_off.append(len(rem_off) - 1)
        rem_row = np.concatenate(rows) if rows else np.zeros(0, np.int64)
        add = np.concatenate(adds) if adds else np.zeros((0, 3))
        return (np.asarray(grp_off, np.int64), np.asarray(rem_off, np.int64), np.ascontiguousarray(rem_row, np.int32),
                np.asarray(add_off, np.int64), np.ascontiguousarray(add[:, 0], np.int32),
                np.ascontiguousarray(add[:, 1], np.int32), np.ascontiguousarray(add[:, 2], np.float32))

    def get_edit_influence(self, test_indices, edits, K=0, first_order=True, dtheta=False):
        """Joint effect of EDIT SETS -- training ratings removed and hypothetical ratings added
        together -- on the predictions of test ratings (one fia_edit_influence call).  edits[q] is
        a sequence of groups of test rating test_indices[q]; a group is a pair (remove_rows,
        add_triples): an integer array of train rows and an array-like [m, 3] of (user, item,
        rating), either may be empty.  For each group, with R the removals and A the additions,

            edit        = v . (H - H_R + H_A)^-1 (b_R - b_A)     the edited system, solved again
            first_order = (H^-1 v) . (b_R - b_A)

        (include/fia.h): the predicted change of r-hat(u, i) once R is removed and A is added.
        With no additions edit is get_group_influence's group; a single addition gives minus
        get_candidate_newton_batch's value; replacing a rating is one removal and one addition on
        the same pair.  A removed row sharing neither the test rating's user nor its item
        contributes nothing; an addition counts once.  len(edits), the pairs, integer rows and ids,
        their ranges, duplicate removals inside a group and K (an integer in [0, FIA_MAX_TOPK])
        are checked on the host (ValueError) before any GPU call.  Returns dict(grp_offsets int64
        [Q+1], edit float64 [G], first_order float64 [G] or None, dtheta float64 [G, D] in the
        reference theta order or None, topk_pos int64 [Q, K] and topk_val float64 [Q, K] or None:
        the K groups of largest |edit| per test rating as positions inside edits[q], -1 / NaN
        where it has fewer than K groups) as numpy arrays.  The large-k models raise FIAError
        (unsupported)."""
        Q = len(test_indices)
        go, ro, rr, ao, au, ai, ay = self._checked_edits(Q, edits)
        if isinstance(K, bool) or int(K) != K or not 0 <= int(K) <= _lib.FIA_MAX_TOPK:
            raise ValueError("K must be in [0, %d]" % _lib.FIA_MAX_TOPK)
        K = int(K)
        D = self._host_num_params()
        import torch
        G = ro.size - 1
        qu, qi = self._query_tensors(test_indices)
        dev = self.ctx.torch_device
        # (the count rejects query ids out of range and queries outside a prepare_for cover)
        self.ctx.count_related(qu, qi)
        dv = lambda a, dt: torch.from_numpy(a).to(dev) if a.size else torch.empty(1, dtype=dt, device=dev)[:0]
        f64 = lambda m: torch.empty(max(m, 1), dtype=torch.float64, device=dev)
        ed = f64(G)
        fo = f64(G) if first_order else None
        dth = f64(G * D) if dtheta else None
        tp = torch.empty(max(Q * K, 1), dtype=torch.int64, device=dev) if K else None
        tv = f64(Q * K) if K else None
        self.ctx.edit_influence(qu, qi, torch.from_numpy(go).to(dev), torch.from_numpy(ro).to(dev),
                                dv(rr, torch.int32), torch.from_numpy(ao).to(dev), dv(au, torch.int32),
                                dv(ai, torch.int32), dv(ay, torch.float32), ed, fo, dth, K, tp, tv)
        return dict(grp_offsets=go, edit=ed[:G].cpu().numpy(),
                    first_order=fo[:G].cpu().numpy() if first_order else None,
                    dtheta=dth[:G * D].cpu().numpy().reshape(G, D) if dtheta else None,
                    topk_pos=tp[:Q * K].cpu().numpy().reshape(Q, K) if K else None,
                    topk_val=tv[:Q * K].cpu().numpy().reshape(Q, K) if K else None)

    def _checked_self_rows(self, train_indices, K, full):
        """Host validation of get_self_influence (no GPU call): returns (rows, K) with rows the
        int32 [n] train rows, or None for every train row, or raises ValueError."""
        if isinstance(K, bool) or int(K) != K or not 0 <= int(K) <= _lib.FIA_MAX_TOPK:
            raise ValueError("K must be in [0, %d]" % _lib.FIA_MAX_TOPK)
        if not full and int(K) == 0:
            raise ValueError("nothing to return: full=False needs K > 0")
        if train_indices is None:
            return None, int(K)
        r = np.asarray(train_indices)
        if r.size == 0:
            r = np.zeros(0, np.int64)
        if r.ndim != 1:
            raise ValueError("train_indices must be a 1-d array of train rows")
        if r.dtype.kind not in "iu":
            raise ValueError("train rows must be integers (got dtype %s)" % r.dtype)
        n_train = int(self.num_train_examples)
        if r.size and (r.min() < 0 or r.max() >= n_train):
            raise ValueError("train rows must lie in [0, %d)" % n_train)
        return np.ascontiguousarray(r, np.int32), int(K)

    def get_self_influence(self, train_indices=None, K=0, full=True):
        """Self-influence (leverage) of training ratings: the effect of each listed rating on its
        OWN prediction (one fia_self_influence call; the scan for noisy or injected ratings).
        For train row j = (a, b, y), with the system of the query (a, b):

            first_order = (H^-1 v) . b_j            the sum of j's two influences in its own related list
            newton      = v . (H - H_j)^-1 b_j      the system without j's curvature, solved again
            error       = r-hat(a, b) - y

        (include/fia.h; get_group_influence of the pair (a, b) with the single group {j}).  Sign
        convention: that of get_influence_on_test_loss -- the predicted change of r-hat(a, b)
        when the rating is removed.  The self-influence on the row's own squared error
        (r-hat - y)^2 is 2 * error * newton.
        train_indices: integer train rows (1-d, in [0, num_train_examples), duplicates allowed),
        or None for every train row in order.  K in [0, FIA_MAX_TOPK]: also the K positions of
        largest |newton| (ties to the lower position).  These, and full=False with K == 0, are
        checked on the host (ValueError) before any GPU call.  Needs a full prepare (not
        prepare_for).  Returns numpy arrays: with full dict(rows int64 [n], first_order, newton,
        error float64 [n]); with K topk_pos int64 [K] (position in train_indices), topk_idx int64
        [K] (train row), topk_val float64 [K] (signed newton), -1 / -1 / NaN in unused slots."""
        rows, K = self._checked_self_rows(train_indices, K, full)
        import torch
        dev = self.ctx.torch_device
        n = self.ctx.n_train if rows is None else rows.size
        d_rows = None
        if rows is not None:
            d_rows = torch.from_numpy(rows).to(dev) if n else torch.empty(1, dtype=torch.int32, device=dev)[:0]
        f64 = lambda m: torch.empty(max(m, 1), dtype=torch.float64, device=dev)
        i64 = lambda m: torch.empty(max(m, 1), dtype=torch.int64, device=dev)
        fo, nw, er = (f64(n), f64(n), f64(n)) if full else (None, None, None)
        tp, ti, tv = (i64(K), i64(K), f64(K)) if K else (None, None, None)
        self.ctx.self_influence(d_rows, fo, nw, er, K, tp, ti, tv)
        out = {}
        if full:
            out["rows"] = np.arange(n, dtype=np.int64) if rows is None else rows.astype(np.int64)
            out["first_order"] = fo[:n].cpu().numpy()
            out["newton"] = nw[:n].cpu().numpy()
            out["error"] = er[:n].cpu().numpy()
        if K:
            out["topk_pos"] = tp[:K].cpu().numpy()
            out["topk_idx"] = ti[:K].cpu().numpy()
            out["topk_val"] = tv[:K].cpu().numpy()
        return out

    def get_newton_influence_batch(self, test_indices, K=1, full=True):
        """Newton-corrected influence of EVERY related rating of many test ratings (one
        fia_query_batch_newton call): per related position p of test rating q, with train row j,

            newton[offsets[q] + p] = v . (H - H_j)^-1 b_j

        -- get_influence_batch's influence with the rating's own curvature taken out of the system
        (get_group_influence of the single group {j}; include/fia.h), from one factorisation per
        query.  A train row that is the test pair itself holds the same value at both of its
        positions.  test_indices must be a 1-d sequence of integers, K in [0, FIA_MAX_TOPK];
        these, and full=False with K == 0, are checked on the host (ValueError) before any GPU
        call.  Returns numpy arrays shaped as get_influence_batch's: offsets int64 [Q + 1]; with
        full rel_idx int64 and newton float64 [total]; with K topk_pos, topk_idx int64 [Q, K] and
        topk_val float64 [Q, K] by |newton| (ties to the lower position, -1 / NaN in unused slots)."""
        if isinstance(K, bool) or int(K) != K or not 0 <= int(K) <= _lib.FIA_MAX_TOPK:
            raise ValueError("K must be in [0, %d]" % _lib.FIA_MAX_TOPK)
        K = int(K)
        if not full and K == 0:
            raise ValueError("nothing to return: full=False needs K > 0")
        t = np.asarray(test_indices)
        if t.size == 0:
            t = np.zeros(0, np.int64)
        if t.ndim != 1:
            raise ValueError("test_indices must be a 1-d sequence of test rows")
        if t.dtype.kind not in "iu":
            raise ValueError("test rows must be integers (got dtype %s)" % t.dtype)
        if t.size and t.min() < 0:
            raise ValueError("test rows must be >= 0")
        import torch
        qu, qi = self._query_tensors([int(v) for v in t])
        Q = qu.numel()
        dev = self.ctx.torch_device
        offsets, total = self.ctx.count_related(qu, qi)
        rel = torch.empty(max(total, 1), dtype=torch.int32, device=dev) if full else None
        nw = torch.empty(max(total, 1), dtype=torch.float64, device=dev) if full else None
        tp = torch.empty(max(Q * K, 1), dtype=torch.int64, device=dev) if K else None
        ti = torch.empty(max(Q * K, 1), dtype=torch.int64, device=dev) if K else None
        tv = torch.empty(max(Q * K, 1), dtype=torch.float64, device=dev) if K else None
        self.ctx.query_batch_newton(qu, qi, offsets, total, rel, nw, K, tp, ti, tv)
        out = dict(offsets=offsets.cpu().numpy())
        if full:
            out["rel_idx"] = rel[:total].cpu().numpy().astype(np.int64)
            out["newton"] = nw[:total].cpu().numpy()
        if K:
            out["topk_pos"] = tp[:Q * K].cpu().numpy().reshape(Q, K)
            out["topk_idx"] = ti[:Q * K].cpu().numpy().reshape(Q, K)
            out["topk_val"] = tv[:Q * K].cpu().numpy().reshape(Q, K)
        return out

    def _checked_other_items(self, test_indices, other_items, distinct=False):
        """Host validation of the second items of pair queries (no GPU call): int32 [Q], one
        in-range item per test rating -- with `distinct`, never the test rating's own item -- or
        ValueError."""
        j = np.asarray(other_items)
        if j.size == 0:
            j = np.zeros(0, np.int64)
        if j.ndim != 1 or j.size != len(test_indices):
            raise ValueError("other_items must hold one item per test index (%d)" % len(test_indices))
        if j.dtype.kind not in "iu":
            raise ValueError("other_items must be integers (got dtype %s)" % j.dtype)
        j = j.astype(np.int64)
        if j.size and (j.min() < 0 or j.max() >= self.num_items):
            raise ValueError("other_items must lie in [0, %d)" % self.num_items)
        if distinct:
            for t, b in zip(test_indices, j):
                if self._test_pair(t)[1] == b:
                    raise ValueError("other_items[t] must differ from the test rating's own item (test row %s)" % t)
        return np.ascontiguousarray(j, np.int32)

    def get_pair_influence_batch(self, test_indices, other_items, K=1, full=True, return_x=True):
        """Which ratings put item i above item j for a user (one fia_pair_batch call): query t is
        the test rating (u_t, i_t) against j = other_items[t], and the explained number is the gap
        d = r-hat(u, i) - r-hat(u, j).  Its system is its own -- theta_t = (theta_u, theta_i,
        theta_j), the related list R_u ++ C_i ++ C_j, one Hessian, one solve (include/fia.h) -- not
        the difference of two get_influence_batch results.  influence[offsets[t] + p] is the
        predicted change of d when the p-th rating of that list is removed.  The length of
        other_items, integer in-range items, j != i_t and K (an integer in [0, FIA_MAX_TOPK]) are
        checked on the host (ValueError) before any GPU call.  Returns dict(offsets int64 [Q + 1],
        diff float64 [Q]; with full rel_idx int64 and influence float64 [total]; with return_x x
        float64 [Q, 3 D / 2] in the extended reference theta order (MF [p_u, q_i, q_j, b_u, b_i,
        b_j], NCF [Pm_u, Qm_i, Qm_j, Pg_u, Qg_i, Qg_j]); with K topk_pos, topk_idx int64 [Q, K] and
        topk_val float64 [Q, K] by |influence|, ties to the lower position, -1 / -1 / NaN in unused
        slots) as numpy arrays.  MF k = 64, NCF k = 32 and the large-k models raise FIAError
        (unsupported)."""
        if isinstance(K, bool) or int(K) != K or not 0 <= int(K) <= _lib.FIA_MAX_TOPK:
            raise ValueError("K must be in [0, %d]" % _lib.FIA_MAX_TOPK)
        K = int(K)
        oj = self._checked_other_items(test_indices, other_items, distinct=True)
        import torch
        qu, qi = self._query_tensors(test_indices)
        Q = qu.numel()
        dev = self.ctx.torch_device
        qj = torch.from_numpy(oj).to(dev) if Q else torch.empty(1, dtype=torch.int32, device=dev)[:0]
        # (the count rejects query ids out of range and entities outside a prepare_for cover)
        offsets, total = self.ctx.count_related_pair(qu, qi, qj)
        D3 = 3 * self._host_num_params() // 2
        f64 = lambda m: torch.empty(max(m, 1), dtype=torch.float64, device=dev)
        i64 = lambda m: torch.empty(max(m, 1), dtype=torch.int64, device=dev)
        rel = torch.empty(max(total, 1), dtype=torch.int32, device=dev) if full else None
        infl = f64(total) if full else None
        x = f64(Q * D3) if return_x else None
        diff = f64(Q)
        tp, ti, tv = (i64(Q * K), i64(Q * K), f64(Q * K)) if K else (None, None, None)
        self.ctx.pair_batch(qu, qi, qj, offsets, total, rel, infl, x, diff, K, tp, ti, tv)
        out = dict(offsets=offsets.cpu().numpy(), diff=diff[:Q].cpu().numpy())
        if full:
            out["rel_idx"] = rel[:total].cpu().numpy().astype(np.int64)
            out["influence"] = infl[:total].cpu().numpy()
        if return_x:
            out["x"] = x[:Q * D3].cpu().numpy().reshape(Q, D3)
        if K:
            out["topk_pos"] = tp[:Q * K].cpu().numpy().reshape(Q, K)
            out["topk_idx"] = ti[:Q * K].cpu().numpy().reshape(Q, K)
            out["topk_val"] = tv[:Q * K].cpu().numpy().reshape(Q, K)
        return out

    def _checked_flip_args(self, n_queries, margin, max_set):
        """Host validation of get_flip_sets' margin and max_set (no GPU call): (float64 [Q] or None,
        int) or ValueError."""
        if isinstance(max_set, bool) or int(max_set) != max_set or not 1 <= int(max_set) <= _lib.FIA_FLIP_MAX_SET:
            raise ValueError("max_set must be an integer in [1, %d]" % _lib.FIA_FLIP_MAX_SET)
        if margin is None:
            return None, int(max_set)
        mg = np.asarray(margin, np.float64)
        if mg.ndim == 0:
            mg = np.full(n_queries, float(mg))
        if mg.ndim != 1 or mg.size != n_queries:
            raise ValueError("margin must be a number or hold one value per test index (%d)" % n_queries)
        if not (mg >= 0.0).all():
            raise ValueError("margin must be >= 0 (and not NaN)")
        return np.ascontiguousarray(mg), int(max_set)

    def get_flip_sets(self, test_indices, other_items, margin=None, max_set=16, return_dtheta=False):
        """The smallest set of a user's own ratings that puts item j above item i (one fia_pair_flip
        call): query t is the test rating (u_t, i_t) against j = other_items[t].  The user's
        ratings of other items with a negative fia_pair_batch value are sorted ascending (ties to
        the lower list position) and taken while fewer than max_set are taken and diff + margin +
        their running sum >= 0 -- ACCENT's greedy first-order set -- and the re-solved system with
        the set removed says what it really does (include/fia.h).  margin: None (0), a number or
        one value >= 0 per query.  The arguments are checked on the host (ValueError) and the batch
        through the pair count (bad ids and a query outside a prepare_for cover raise as they do
        for get_pair_influence_batch) before the call.  Returns dict(diff, margin, first_order,
        newton float64 [Q]; set_size int64 [Q]; sets, set_vals: lists of Q arrays of their true
        length (train rows int64, values float64); flipped_first_order = diff + first_order <
        -margin and flipped_newton = diff + newton < -margin, bool [Q]; with return_dtheta dtheta
        float64 [Q, 3 D / 2] in the extended reference theta order) as numpy arrays.  MF k = 64,
        NCF k = 32 and the large-k models raise FIAError (unsupported)."""
        oj = self._checked_other_items(test_indices, other_items, distinct=True)
        mg, max_set = self._checked_flip_args(len(test_indices), margin, max_set)
        import torch
        qu, qi = self._query_tensors(test_indices)
        Q = qu.numel()
        dev = self.ctx.torch_device
        qj = torch.from_numpy(oj).to(dev) if Q else torch.empty(1, dtype=torch.int32, device=dev)[:0]
        # (the count rejects query ids out of range and entities outside a prepare_for cover)
        self.ctx.count_related_pair(qu, qi, qj, want_total=True)
        D3 = 3 * self._host_num_params() // 2
        f64 = lambda m: torch.empty(max(m, 1), dtype=torch.float64, device=dev)
        i32 = lambda m: torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        dmg = torch.from_numpy(mg).to(dev) if (mg is not None and Q) else None
        size, rows, vals = i32(Q), i32(Q * max_set), f64(Q * max_set)
        first, newton, diff = f64(Q), f64(Q), f64(Q)
        dth = f64(Q * D3) if return_dtheta else None
        self.ctx.pair_flip(qu, qi, qj, max_set, dmg, size, rows, vals, first, newton, dth, diff)
        size = size[:Q].cpu().numpy().astype(np.int64)
        rows = rows[:Q * max_set].cpu().numpy().astype(np.int64).reshape(Q, max_set)
        vals = vals[:Q * max_set].cpu().numpy().reshape(Q, max_set)
        mgv = np.zeros(Q) if mg is None else mg
        out = dict(diff=diff[:Q].cpu().numpy(), margin=mgv, first_order=first[:Q].cpu().numpy(),
                   newton=newton[:Q].cpu().numpy(), set_size=size,
                   sets=[rows[q, :max(size[q], 0)].copy() for q in range(Q)],
                   set_vals=[vals[q, :max(size[q], 0)].copy() for q in range(Q)])
        out["flipped_first_order"] = out["diff"] + out["first_order"] < -mgv
        out["flipped_newton"] = out["diff"] + out["newton"] < -mgv
        if return_dtheta:
            out["dtheta"] = dth[:Q * D3].cpu().numpy().reshape(Q, D3)
        return out

    def get_counterfactual_explanation(self, test_idx, alternatives, margin=0.0, max_set=16, verified=True):
        """ACCENT's outer loop for one test rating (u, i): one get_flip_sets batch over (u, i, j) for
        j in `alternatives`, and among the alternatives whose set flips -- judged by the re-solved
        system (flipped_newton) with `verified`, else to first order -- the one with the fewest
        rows, ties to the earlier alternative.  Returns dict(item, rows, vals: the chosen
        alternative, its train rows and their values, or None / None / None when no set flips;
        index: its position in `alternatives` or -1; table: get_flip_sets' result, one entry per
        alternative)."""
        alts = np.asarray(alternatives)
        if alts.ndim != 1 or alts.size == 0:
            raise ValueError("alternatives must be a non-empty 1-d sequence of items")
        table = self.get_flip_sets([test_idx] * alts.size, alts, margin=margin, max_set=max_set)
        flipped = table["flipped_newton"] if verified else table["flipped_first_order"]
        best = -1
        for a in range(alts.size):
            if flipped[a] and (best < 0 or table["set_size"][a] < table["set_size"][best]):
                best = a
        if best < 0:
            return dict(item=None, rows=None, vals=None, index=-1, table=table)
        return dict(item=int(alts[best]), rows=table["sets"][best], vals=table["set_vals"][best], index=best,
                    table=table)

    def _checked_slates(self, users, slates, weights):
        """The host-side checks of get_slate_influence_batch (ValueError): returns (users int32 [Q],
        slate_offsets int64 [Q + 1], items int32 [total], weights float64 [total])."""
        def ints(a, what):
            a = np.asarray(a)
            if a.ndim != 1 or (a.size and (a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer))):
                raise ValueError("%s must be a 1-d sequence of integers (got dtype %s, shape %s)" % (what, a.dtype,
                                                                                                    a.shape))
            return a.astype(np.int64)
        u = ints(users, "users")
        if u.size and (u.min() < 0 or u.max() >= self.num_users):
            raise ValueError("users must lie in [0, %d)" % self.num_users)
        if len(slates) != u.size:
            raise ValueError("%d users but %d slates" % (u.size, len(slates)))
        if weights is not None and len(weights) != u.size:
            raise ValueError("%d users but %d weight lists" % (u.size, len(weights)))
        items, wts, off = [], [], [0]
        for q in range(u.size):
            it = ints(slates[q], "slates[%d]" % q)
            if not 1 <= it.size <= _lib.FIA_SLATE_MAX_ITEMS:
                raise ValueError("slates[%d] holds %d items, not in [1, %d]" % (q, it.size, _lib.FIA_SLATE_MAX_ITEMS))
            if it.min() < 0 or it.max() >= self.num_items:
                raise ValueError("slates[%d] must lie in [0, %d)" % (q, self.num_items))
            if np.unique(it).size != it.size:
                raise ValueError("slates[%d] repeats an item" % q)
            if weights is None:
                w = 1.0 / np.log2(np.arange(it.size) + 2.0)        # DCG's discount, rank from 0
            else:
                try:
                    w = np.asarray(weights[q], np.float64)
                except (TypeError, ValueError):
                    raise ValueError("weights[%d] must be numbers" % q)
                if w.shape != it.shape:
                    raise ValueError("weights[%d] holds %s values for %d items" % (q, w.shape, it.size))
                if not np.isfinite(w).all():
                    raise ValueError("weights[%d] must be finite" % q)
            items.append(it)
            wts.append(w)
            off.append(off[-1] + it.size)
        cat = lambda parts, dt: np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0), dt)
        return np.ascontiguousarray(u, np.int32), np.asarray(off, np.int64), cat(items, np.int32), cat(wts, np.float64)

    def get_slate_influence_batch(self, users, slates, weights=None, K=1, full=True, return_x=True):
        """Which ratings shape a user's ranked list (one fia_slate_batch call): query t is user
        users[t] (a user id, not a test index) with the ranked items slates[t] (1 to
        FIA_SLATE_MAX_ITEMS distinct item ids) and the explained number is the weighted sum
        f = sum_l weights[t][l] * r-hat(u, i_l); the default weights are DCG's discount
        1 / log2(rank + 2), rank from 0.  Its system is its own -- theta_t = (theta_u, theta_i1 ..
        theta_im), the related list R_u ++ C_i1 ++ .. ++ C_im, one Hessian, one solve
        (include/fia.h) -- not the weighted sum of get_influence_batch results.
        influence[offsets[t] + p] is the predicted change of f when the p-th rating of that list is
        removed.  Equal lengths, integer in-range ids, the slate lengths, distinct items per slate,
        finite weights and K (an integer in [0, FIA_MAX_TOPK]) are checked on the host (ValueError)
        before any GPU call.  Returns dict(offsets int64 [Q + 1], value float64 [Q]; with full
        rel_idx int64 and influence float64 [total]; with return_x x, a list of Q float64 vectors
        [(m_t + 1) Ds] in the extended reference theta order (MF [p_u, q_1 .. q_m, b_u, b_1 .. b_m],
        NCF [Pm_u, Qm_1 .., Pg_u, Qg_1 ..]); with K topk_pos, topk_idx int64 [Q, K] and topk_val
        float64 [Q, K] by |influence|, ties to the lower position, -1 / -1 / NaN in unused slots) as
        numpy arrays.  Every small-k size is served; the large-k models raise FIAError
        (unsupported)."""
        if isinstance(K, bool) or int(K) != K or not 0 <= int(K) <= _lib.FIA_MAX_TOPK:
            raise ValueError("K must be in [0, %d]" % _lib.FIA_MAX_TOPK)
        K = int(K)
        u, soff, items, wts = self._checked_slates(users, slates, weights)
        import torch
        Q, TI = u.size, items.size
        dev = self.ctx.torch_device
        up = lambda a: torch.from_numpy(a).to(dev) if a.size else torch.empty(1, dtype=torch.from_numpy(a).dtype,
                                                                              device=dev)[:0]
        qu, so, it, wt = up(u), torch.from_numpy(soff).to(dev), up(items), up(wts)
        # (the count rejects entities outside a prepare_for cover)
        offsets, total = self.ctx.count_related_slate(qu, so, it)
        Ds = self._host_num_params() // 2
        f64 = lambda m: torch.empty(max(m, 1), dtype=torch.float64, device=dev)
        i64 = lambda m: torch.empty(max(m, 1), dtype=torch.int64, device=dev)
        rel = torch.empty(max(total, 1), dtype=torch.int32, device=dev) if full else None
        infl = f64(total) if full else None
        x = f64(Ds * (TI + Q)) if return_x else None
        value = f64(Q)
        tp, ti, tv = (i64(Q * K), i64(Q * K), f64(Q * K)) if K else (None, None, None)
        self.ctx.slate_batch(qu, so, it, wt, offsets, total, rel, infl, x, value, K, tp, ti, tv)
        out = dict(offsets=offsets.cpu().numpy(), value=value[:Q].cpu().numpy())
        if full:
            out["rel_idx"] = rel[:total].cpu().numpy().astype(np.int64)
            out["influence"] = infl[:total].cpu().numpy()
        if return_x:
            xs = x[:Ds * (TI + Q)].cpu().numpy()
            out["x"] = [xs[Ds * (soff[q] + q):Ds * (soff[q + 1] + q + 1)].copy() for q in range(Q)]
        if K:
            out["topk_pos"] = tp[:Q * K].cpu().numpy().reshape(Q, K)
            out["topk_idx"] = ti[:Q * K].cpu().numpy().reshape(Q, K)
            out["topk_val"] = tv[:Q * K].cpu().numpy().reshape(Q, K)
        return out

    def _predict_device(self, qu, qi):
        """r-hat(u, i) in fp64 on the device from the uploaded (float32) parameter tables."""
        import torch
        k = int(self.embedding_size)
        u, i = qu.long(), qi.long()
        t = [p.double() for p in self._dev_params]
        if self.MODEL_ID == _lib.FIA_MODEL_MF:
            return (t[0].view(-1, k)[u] * t[1].view(-1, k)[i]).sum(1) + t[2][u] + t[3][i] + t[4][0]
        h = k // 2
        x0 = torch.cat([t[0].view(-1, k)[u], t[1].view(-1, k)[i]], 1)
        h1 = torch.relu(x0 @ t[4].view(2 * k, k) + t[5])
        h2 = torch.relu(h1 @ t[6].view(k, h) + t[7])
        gmf = t[2].view(-1, k)[u] * t[3].view(-1, k)[i]
        return h2 @ t[8][:h] + gmf @ t[8][h:] + t[9][0]

    def get_influence_on_test_set_loss(self, test_indices, K=0):
        """The Koh-Liang aggregate over a test set: the influence of every training rating on the
        mean squared test error L = (1 / Q) sum_q (r-hat(u_q, i_q) - y_q)^2, to first order

            total[j] = sum_q 2 (r-hat(u_q, i_q) - y_q) / Q * (influence of row j on r-hat(u_q, i_q))

        = get_total_influence(test_indices, weights) with weights[q] = 2 (r-hat_q - y_q) / Q,
        y_q from data_sets["test"].labels and r-hat_q computed in fp64 on the device from the
        uploaded tables.  Sign: the per-query influence is the predicted change of r-hat(test)
        when the training rating is REMOVED (experiments.test_retraining compares it with r-hat
        after leave-one-out retraining minus r-hat before), so total[j] > 0 means that removing
        rating j raises the mean test loss -- the rating helps -- and total[j] < 0 that removing
        it lowers the loss.  Returns get_total_influence's dict plus weights [Q]."""
        Q = len(test_indices)
        qu, qi = self._query_tensors(test_indices)
        y = np.asarray(self.data_sets["test"].labels, np.float64).reshape(-1)[np.asarray(test_indices, np.int64)]
        if Q:
            w = (2.0 * (self._predict_device(qu, qi).cpu().numpy() - y) / Q)
        else:
            w = np.zeros(0)
        out = self.get_total_influence(test_indices, weights=w, K=K, full=True)
        out["weights"] = w
        return out

    def _score_one_query_candidates(self, test_index, x, X, Y):
        off = np.array([0, len(Y)], np.int64)
        return self.get_candidate_influence_batch([test_index], off, X, Y, K=0, full=True,
                                                  inverse_hvp=x)["influence"]

    def get_influence_on_test_loss(self, test_indices, train_idx, approx_type="cg", approx_params=None,
                                   force_refresh=True, test_description=None, loss_type="normal_loss",
                                   X=None, Y=None):
        """Predicted change of r-hat(test pair) when each related training rating is
        removed (mf:164-251, ncf:193-280).  Returns float64[n] aligned with
        self.train_indices_of_test_case.

        Phantom points (train_idx None with X [M, 2] and Y [M] given, mf:228-235): the call
        runs as usual up to and including the inverse HVP (cache file, save_inverse_hvp and the
        side-effect attributes alike) and returns float64[len(Y)], the influence of each
        hypothetical rating (X[c, 0], X[c, 1], Y[c]) as get_candidate_influence_batch defines
        it -- divided by the query's related-set size, not by num_train_examples.

        Differences from the reference, by design: the inverse HVP is the exact fp64
        solve (the reference's fmin_ncg approximates it, mf:424-431); errors raise
        ValueError (the reference raises tuples, mf:173-177); the reference's own
        phantom-point branch is shape-inconsistent (it dots the restricted inverse HVP with a
        full-parameter gradient) and cannot run."""
        phantom = train_idx is None
        if phantom:
            if X is None or Y is None:
                raise ValueError("X and Y must be specified if using phantom points.")
            if X.shape[0] != len(Y):
                raise ValueError("X and Y must have the same length.")
        elif X is not None or Y is not None:
            raise ValueError("X and Y cannot be specified if train_idx is specified.")
        if approx_type == "lissa":
            # gnn:503-508 dispatches 'lissa' to get_inverse_hvp_lissa (gnn:511-544); this
            # build has one solver, the exact fp64 LDL^T, and does not pretend otherwise
            raise NotImplementedError("approx_type='lissa' is not provided: the inverse HVP is the exact fp64 "
                                      "solve (use approx_type='cg')")
        if approx_type != "cg":
            raise ValueError("approx_type must be 'cg' or 'lissa'")
        if loss_type != "normal_loss":
            raise ValueError("Loss must be normal")
        assert len(test_indices) == 1
        if phantom:     # shapes and id ranges, on the host, before any GPU call
            self._checked_candidates(1, np.array([0, len(Y)], np.int64), X, Y)
        t0 = time.time()
        self.test_index = test_indices[0]
        self.test_u, self.test_i = self._test_pair(self.test_index)
        # the three RQ2 stage timers (mf:224-250) come from the library's HIP-event phases of
        # this one call: inverse HVP = related lists + Hessian assembly + solve, multiplying =
        # per-rating scoring (+ the fused top-K)
        if test_description is None:
            test_description = test_indices
        fname = os.path.join(self.train_dir, "%s-%s-%s-test-%s.npz" % (
            self.model_name, approx_type, loss_type, test_description))
        # the reference's cached inverse HVP (mf:210-214): with force_refresh False and the
        # file present, its vector replaces the solve (scored on the GPU, fia_query_batch_x)
        # Only a flat float64 vector of this model's D values is accepted: the reference
        # itself saves a ragged per-block list (mf:221), which numpy stores as an object
        # array that allow_pickle=False refuses -- such a file, or one of another size, is
        # treated as absent and the solve runs (pickles are never loaded), and is left as it is:
        # the reference never overwrites its cache file when force_refresh is False.
        cached = None
        unusable = False
        if not force_refresh and os.path.exists(fname):
            try:
                with np.load(fname, allow_pickle=False) as z:
                    arr = np.asarray(z["inverse_hvp"])
                if arr.dtype.kind == "f" and arr.size == self.ctx.num_params():
                    cached = arr.astype(np.float64).reshape(1, -1)
            except (ValueError, KeyError, OSError):
                cached = None
            unusable = cached is None
            if self.verbose:
                print(("Loaded inverse HVP from %s" if cached is not None else
                       "Ignored unusable inverse HVP file %s") % fname)
        # (the caller's own profiling mask and unread sums are kept: Context.profiled_call)
        res, phases = self.ctx.profiled_call(lambda: self._one_query(self.test_index, cached))
        self.train_indices_of_test_case = res["rel_idx"]
        x = res["x"][0]
        self.num_params = x.size
        self.inverse_hvp = self._split_theta(x)
        if self.save_inverse_hvp and cached is None and not unusable:
            np.savez(fname, inverse_hvp=x)
        if phantom:
            # the hypothetical ratings scored with the same inverse HVP (fia_score_candidates;
            # its kernels add to the 'score' phase of the timers)
            infl, more = self.ctx.profiled_call(lambda: self._score_one_query_candidates(self.test_index, x, X, Y))
            phases = {p: (phases[p][0] + more[p][0], phases[p][1] + more[p][1]) for p in phases}
            self.last_timing = rq2_timing(phases, infl.size, time.time() - t0, log=print if self.verbose else None)
            return infl
        self.last_timing = rq2_timing(phases, res["influence"].size, time.time() - t0,
                                      log=print if self.verbose else None)
        return res["influence"]

    def _one_query(self, test_index, inverse_hvp=None):
        """One test rating, as get_influence_batch([test_index], K=0) returns it, with a single
        host synchronisation (the reference times each query, RQ2.py:53,57): the related-set size
        from host degree counts instead of a count round trip, persistent device and pinned host
        buffers, the query pair and every result copied in stream order, one wait at the end.
        Falls back to get_influence_batch when its checks are needed: ids out of range (the
        count raises) or caches built by prepare_for (the cover check raises)."""
        import torch
        u, i = self._test_pair(test_index)
        if not (0 <= u < self.num_users and 0 <= i < self.num_items) or not self.ctx.full_prepared:
            return self.get_influence_batch([test_index], K=0, full=True, return_x=True, inverse_hvp=inverse_hvp)
        n = int(self._deg_u[u] + self._deg_i[i])
        D = self.ctx.num_params()
        b = getattr(self, "_one_bufs", None)
        if b is None or b["cap"] < max(n, 1) or b["D"] != D:
            cap = max(n, 1024, 2 * (b["cap"] if b else 0))
            b = self._one_alloc(cap, D)
        b["hin"].numpy()[:2] = (u, i)
        b["din"][:8].copy_(b["hin_all"][:8], non_blocking=True)
        qu, qi = b["q"][0:1], b["q"][1:2]
        self.ctx.count_related(qu, qi, b["off"], want_total=False)
        if inverse_hvp is not None:
            xin = np.ascontiguousarray(np.asarray(inverse_hvp, np.float64).reshape(-1))
            if xin.size != D:
                raise ValueError("inverse_hvp must hold %d values" % D)
            b["hxin"].numpy()[:] = xin
            b["din"][8:].copy_(b["hin_all"][8:], non_blocking=True)
            self.ctx.query_batch_x(qu, qi, b["off"], n, b["xin"], b["rel"], b["infl"], 0, None, None, None)
        else:
            self.ctx.query_batch(qu, qi, b["off"], n, b["rel"], b["infl"], b["x"], 0, None, None, None)
        # every result in one copy (offsets, rows, influence and x share one device block)
        b["hout"].copy_(b["dout"], non_blocking=True)
        torch.cuda.current_stream(self.ctx.torch_device).synchronize()
        hv = b["hviews"]
        x = hv["x"] if inverse_hvp is None else xin
        return dict(offsets=hv["off"].copy(), rel_idx=hv["rel"][:n].astype(np.int64),
                    influence=hv["infl"][:n].copy(), x=np.array(x, np.float64).reshape(1, D))

    def _one_alloc(self, cap, D):
        """_one_query's persistent blocks: in = {u, i} (+ a given x), out = {offsets[2], x[D],
        influence[cap], rows[cap]} -- one device block and one pinned host block each way."""
        import torch
        dev = self.ctx.torch_device
        n_in = 8 + 8 * D                         # two int32 ids (8 B), then x_in
        o_off, o_x = 0, 16
        o_infl = o_x + 8 * D
        o_rel = o_infl + 8 * cap
        n_out = o_rel + 4 * cap
        din = torch.empty(n_in, dtype=torch.uint8, device=dev)
        hin = torch.empty(n_in, dtype=torch.uint8, pin_memory=True)
        dout = torch.empty(n_out, dtype=torch.uint8, device=dev)
        hout = torch.empty(n_out, dtype=torch.uint8, pin_memory=True)
        hnp = hout.numpy()
        b = dict(cap=cap, D=D, din=din, dout=dout,
                 hin=hin[:8].view(torch.int32), hxin=hin[8:].view(torch.float64), hout=hout,
                 q=din[:8].view(torch.int32), xin=din[8:].view(torch.float64),
                 off=dout[o_off:o_off + 16].view(torch.int64), x=dout[o_x:o_x + 8 * D].view(torch.float64),
                 infl=dout[o_infl:o_infl + 8 * cap].view(torch.float64),
                 rel=dout[o_rel:o_rel + 4 * cap].view(torch.int32),
                 hviews=dict(off=hnp[o_off:o_off + 16].view(np.int64), x=hnp[o_x:o_x + 8 * D].view(np.float64),
                             infl=hnp[o_infl:o_infl + 8 * cap].view(np.float64),
                             rel=hnp[o_rel:o_rel + 4 * cap].view(np.int32)))
        b["hin_all"] = hin
        self._one_bufs = b
        return b

    def _split_theta(self, x):
        raise NotImplementedError

    def _theta_blocks(self, u, i):
        raise NotImplementedError
