"""Linear probe: a multinomial logistic regression fitted on frozen embeddings, the supervised yardstick next to the zero-shot figures
(the reference scores a shipped classifier head for it, mmgclip/evaluator.py evaluate_cnn / clf_conf_matrix; a probe fitted here needs
none).  The device evaluates loss and gradient with the fused kernel of csrc/probe_head.hip (`head._HipProbeBackend`): one read of
X per evaluation, no [n,C] temporary, a fixed summation order.

The objective.  With labels y_i in [-1, C) (-1 = ignored), row weights w_i = class_weight[y_i] (1 without a table) and S = sum_i w_i,
    F(W, b) = L / S + (l2 / 2) ||W||_F^2,     L = sum_i w_i (logsumexp_c z_ic - z_{i,y_i}),   z = X W^T + b.
The bias is not regularised.  sklearn's `LogisticRegression(C=...)` minimises C L + ||W||^2 / 2, so its C equals 1 / (l2 * S).

The solver is an L-BFGS of the project's own (`lbfgs_minimize`: two-loop recursion, history 10, backtracking Armijo line search,
W0 = 0) in float64 numpy on the host over the C (D+1) unknowns.  The device only evaluates (L, dW, db): per evaluation the host uploads
W, b in fp32 and reads the fp64 result back; F and its gradient are taken AT those fp32 weights, which are what `fit` keeps.  It is not
scipy's routine, so every rank of a sharded run takes bit-identical steps.  It stops at max_i |grad F| <= gtol or at max_iter.

Sharded (an active `comm`): every rank passes its shard of (X, y); shards may be uneven or empty.  Per evaluation the fp64 result
vector is all-reduced (SUM); S and the balanced class weights come from globally summed label counts, once per fit.  The fitted W, b
are identical on every rank.  They are NOT bit-equal to the unsharded fit: the float sums are regrouped.

`fused=None` takes the kernel for a GPU tensor when `mmg_probe_rows_supported(D, C)`, otherwise the dense torch route
(`dense_evaluate`; always on the CPU); `fused=True` insists on the kernel, `fused=False` on the dense route.  The dense route reads X
twice per evaluation and forms two [n,C] temporaries; it is kept as a method of its own as the yardstick of tools/probe_cost.py and the
tests."""
import numpy as np
import torch

from . import head
from .search import _check_rows

MAX_FUSED_C = 32
HISTORY = 10
ARMIJO_C1 = 1e-4
MAX_BACKTRACKS = 40


def lbfgs_minimize(fun, x0, max_iter, gtol, history=HISTORY):
    """Minimise `fun` (x float64 [m] -> (f, g float64 [m])) from x0: L-BFGS by the two-loop recursion over the last `history` pairs,
    initial scaling s'y / y'y, backtracking (halving) Armijo line search from step 1 (the first step from 1 / ||g||_1).  Stops at
    max|g| <= gtol, after max_iter iterations, or when the line search finds no decrease (the noise floor of `fun`).
    -> (x, f, g, n_iter, converged, n_evaluations).  Pure float64 numpy: the same inputs give the same steps anywhere."""
    x = np.array(x0, dtype=np.float64)
    f, g = fun(x)
    n_eval, pairs = 1, []
    n_iter = 0
    while n_iter < max_iter and np.max(np.abs(g)) > gtol:
        q = g.copy()
        alphas = []
        for s, yv, rho in reversed(pairs):
            a = rho * np.dot(s, q)
            alphas.append(a)
            q -= a * yv
        if pairs:
            s, yv, _ = pairs[-1]
            q *= np.dot(s, yv) / np.dot(yv, yv)
        for (s, yv, rho), a in zip(pairs, reversed(alphas)):
            q += (a - rho * np.dot(yv, q)) * s
        d = -q
        gd = np.dot(g, d)
        if not gd < 0:                                     # not a descent direction (rounding): steepest descent, history dropped
            pairs, d = [], -g
            gd = np.dot(g, d)
        t = 1.0 if pairs else min(1.0, 1.0 / np.sum(np.abs(g)))
        for _ in range(MAX_BACKTRACKS):
            xn = x + t * d
            fn, gn = fun(xn)
            n_eval += 1
            if fn <= f + ARMIJO_C1 * t * gd:
                break
            t *= 0.5
        else:
            break                                          # no decrease at any step: x stays
        s, yv = xn - x, gn - g
        sy = np.dot(s, yv)
        if sy > 1e-12 * np.dot(yv, yv):
            pairs.append((s, yv, 1.0 / sy))
            pairs = pairs[-history:]
        x, f, g = xn, fn, gn
        n_iter += 1
    return x, f, g, n_iter, bool(np.max(np.abs(g)) <= gtol), n_eval


def _check_labels(name, y, n, C=None):
    if not torch.is_tensor(y) or y.ndim != 1 or y.dtype != torch.int64 or y.shape[0] != n:
        raise ValueError(f"{name} must be an int64 vector with one label per row ({n}), got "
                         f"{(tuple(y.shape), y.dtype) if torch.is_tensor(y) else type(y).__name__}")
    if n and (int(y.min()) < -1 or (C is not None and int(y.max()) >= C)):
        raise ValueError(f"{name} must lie in [-1, C) with -1 the ignore label" + (f" (C={C})" if C is not None else "") +
                         f", got {int(y.min())} .. {int(y.max())}")


class LinearProbe:
    def __init__(self, l2=1e-3, max_iter=200, gtol=1e-4, class_weight=None, comm=None, fused=None):
        if isinstance(l2, bool) or not isinstance(l2, (int, float)) or not l2 > 0:
            raise ValueError(f"l2 must be a positive number (the objective is strongly convex in W only then), got {l2!r}")
        if isinstance(max_iter, bool) or not isinstance(max_iter, int) or max_iter < 0:
            raise ValueError(f"max_iter must be a non-negative integer, got {max_iter!r}")
        if isinstance(gtol, bool) or not isinstance(gtol, (int, float)) or not gtol > 0:
            raise ValueError(f"gtol must be a positive number, got {gtol!r}")
        if not (class_weight is None or torch.is_tensor(class_weight) or class_weight == "balanced"):
            raise ValueError(f'class_weight must be None, "balanced" or a [C] tensor, got {class_weight!r}')
        if fused not in (None, True, False):
            raise ValueError(f"fused must be None, True or False, got {fused!r}")
        self.l2, self.max_iter, self.gtol = float(l2), max_iter, float(gtol)
        self.class_weight, self.comm, self.fused = class_weight, comm, fused
        self.weight = self.bias = self.classes = None
        self.n_iter_ = self.converged_ = self.grad_norm_ = self.objective_ = self.n_evaluations_ = None

    @property
    def _sharded(self):
        return self.comm is not None and self.comm.active

    # ---- one evaluation ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def dense_evaluate(X, W, b, y, class_weight=None):
        """The dense torch route, the layout of `head._HipProbeBackend.evaluate`: fp64 [C (D+1) + 1] = dW | db as [C, D+1], then L.
        Two reads of X and two [n,C] temporaries; the per-row losses are fp32, their sum fp64."""
        C, D = W.shape
        z = X @ W.t() + b
        valid = y >= 0
        yc = y.clamp(min=0)
        w = valid.to(z.dtype) if class_weight is None else class_weight[yc] * valid
        lse = torch.logsumexp(z, dim=1)
        L = (w * (lse - z.gather(1, yc[:, None])[:, 0])).double().sum()
        G = torch.softmax(z, dim=1)
        G[torch.arange(X.shape[0], device=X.device), yc] -= 1.0
        G *= w[:, None]
        grad = torch.cat([G.t() @ X, G.sum(dim=0)[:, None]], dim=1)
        return torch.cat([grad.flatten().double(), L.reshape(1)])

    def _use_fused(self, X, C):
        D = X.shape[1]
        ok = X.is_cuda and head._HipProbeBackend.supported(D, C)
        if self.fused is True and not ok:
            raise ValueError(f"fused=True needs a GPU tensor with D % 32 == 0 in [32,1024] and 2 <= C <= {MAX_FUSED_C}; got "
                             f"D={D}, C={C} on {X.device}")
        return ok if self.fused is None else self.fused

    def evaluate(self, X, y, W, b, class_weight=None):
        """The GLOBAL un-normalised (dW | db, L) at the fp32 weights W [C,D], b [C]: fp64 [C (D+1) + 1] on X's device, summed over
        the ranks of an active communicator.  An empty shard adds zeros."""
        C, D = W.shape
        if X.shape[0] == 0:
            out = torch.zeros(C * (D + 1) + 1, device=X.device, dtype=torch.float64)
        elif self._use_fused(X, C):
            out = head._HipProbeBackend.evaluate(X, W, b, y, class_weight)
        else:
            out = self.dense_evaluate(X, W, b, y, class_weight)
        return self.comm.all_reduce_sum(out) if self._sharded else out

    # ---- fit ------------------------------------------------------------------------------------------------------------------------
    def _global_counts(self, y, C):
        counts = torch.bincount(y[y >= 0], minlength=C).to(torch.int64)
        return self.comm.all_reduce_sum(counts) if self._sharded else counts

    def _weights(self, counts, C, device):
        """-> (fp32 [C] table on the device or None, S as a Python float) from the GLOBAL label counts."""
        counts = counts.cpu().double()
        if self.class_weight is None:
            return None, float(counts.sum())
        if torch.is_tensor(self.class_weight):
            cw = self.class_weight.detach().to(dtype=torch.float32, device="cpu")
            if cw.shape != (C,) or bool((cw < 0).any()) or not bool(torch.isfinite(cw).all()):
                raise ValueError(f"class_weight must hold C={C} finite non-negative weights, got {tuple(cw.shape)}")
        else:                                              # "balanced": n / (C * count), sklearn's rule; an absent class weighs 0
            cw = torch.where(counts > 0, counts.sum() / (C * counts.clamp(min=1)), torch.zeros_like(counts)).float()
        return cw.to(device).contiguous(), float((cw.double() * counts).sum())

    def fit(self, X, y, n_classes=None, warm_start=False):
        """Fit on the rows X [n,D] (fp32, contiguous) with int64 labels in [-1, C); C = `n_classes`, or the largest label of all ranks
        plus one.  `warm_start` starts from the weights the object holds (of the same shape) instead of zero.  Returns self."""
        _check_rows("X", X)
        n, D = X.shape
        _check_labels("y", y, n)
        X, y = X.detach(), y.detach().to(X.device).contiguous()
        if n_classes is None:
            top = torch.tensor([int(y.max()) if n else -1], dtype=torch.int64, device=X.device)
            n_classes = int((self.comm.all_gather_rows(top) if self._sharded else top).max()) + 1
        C = int(n_classes)
        if C < 2:
            raise ValueError(f"a probe needs at least two classes, got C={C}")
        _check_labels("y", y, n, C)
        cw, S = self._weights(self._global_counts(y, C), C, X.device)
        if not S > 0:
            raise ValueError("no labelled row with a positive weight: nothing to fit")
        E = C * (D + 1)

        def fun(theta):
            t32 = theta.astype(np.float32).reshape(C, D + 1)
            W = torch.from_numpy(np.ascontiguousarray(t32[:, :D])).to(X.device)
            b = torch.from_numpy(np.ascontiguousarray(t32[:, D])).to(X.device)
            out = self.evaluate(X, y, W, b, cw).cpu().numpy()
            t = t32.astype(np.float64)
            reg = t.copy()
            reg[:, D] = 0.0                                # the bias is not regularised
            return out[E] / S + 0.5 * self.l2 * float(np.sum(reg * reg)), out[:E] / S + self.l2 * reg.reshape(-1)

        theta0 = np.zeros(E, dtype=np.float64)
        if warm_start and self.weight is not None and tuple(self.weight.shape) == (C, D):
            theta0 = torch.cat([self.weight, self.bias[:, None]], dim=1).double().cpu().numpy().reshape(-1)
        theta, f, g, self.n_iter_, self.converged_, self.n_evaluations_ = lbfgs_minimize(fun, theta0, self.max_iter, self.gtol)
        t32 = torch.from_numpy(theta.astype(np.float32).reshape(C, D + 1))
        self.weight, self.bias = t32[:, :D].contiguous().to(X.device), t32[:, D].contiguous().to(X.device)
        self.classes = torch.arange(C, dtype=torch.int64)
        self.objective_, self.grad_norm_ = float(f), float(np.max(np.abs(g)))
        return self

    # ---- prediction -------------------------------------------------------------------------------------------------------------
    def _fitted(self, X):
        if self.weight is None:
            raise RuntimeError("the probe is not fitted: call fit() or load_state_dict() first")
        _check_rows("X", X, self.weight.shape[1])

    def decision_function(self, X):
        """[n,C] fp32 logits X W^T + b.  On the kernel's domain the product is the heads' logit kernel (`head.rows_forward`)."""
        self._fitted(X)
        W, b = self.weight.to(X.device), self.bias.to(X.device)
        if X.shape[0] and self._use_fused(X, W.shape[0]):
            one = torch.ones(1, device=X.device, dtype=torch.float32)
            return head.rows_forward(X.detach(), W, one, 0, True)[2] + b
        return X.detach() @ W.t() + b

    def predict_proba(self, X):
        return torch.softmax(self.decision_function(X), dim=1)

    def predict(self, X):
        """int64 [n]: the class of the largest logit (the lowest index on a tie)."""
        z = self.decision_function(X)
        return self.classes.to(X.device)[torch.argmax(z, dim=1)]

    # ---- model selection -------------------------------------------------------------------------------------------------------
    def sweep(self, X_tr, y_tr, X_val, y_val, l2s, n_classes=None):
        """Fit once per regularisation strength, from the largest l2 downwards, each fit warm-started from the one before, and keep
        the fit with the best validation macro-AUROC (`ZeroShotAUROC` on the class probabilities, global over the ranks); a tie goes to
        the larger l2.  `y_val` is checked like `y`; a validation row with the ignore label -1 is LEFT OUT of the AUROC (handed on,
        `ZeroShotAUROC` would count it as a negative of every class).  `sweep_` holds (l2, auc, n_iter) per fit in the order fitted.
        Returns self, holding the best fit."""
        from .zeroshot_auroc import ZeroShotAUROC
        l2s = sorted({float(v) for v in l2s}, reverse=True)
        if not l2s or not l2s[-1] > 0:
            raise ValueError(f"l2s must be a non-empty collection of positive numbers, got {l2s!r}")
        _check_rows("X_val", X_val, X_tr.shape[1] if torch.is_tensor(X_tr) and X_tr.ndim == 2 else None)
        _check_labels("y_val", y_val, X_val.shape[0], n_classes)
        known = torch.nonzero(y_val.to(X_val.device) >= 0).flatten()
        X_val, y_val = X_val.detach()[known].contiguous(), y_val.to(X_val.device)[known].contiguous()
        best, self.sweep_ = None, []
        for i, l2 in enumerate(l2s):
            self.l2 = l2
            self.fit(X_tr, y_tr, n_classes=n_classes, warm_start=i > 0)
            if i == 0:
                _check_labels("y_val", y_val, y_val.shape[0], self.weight.shape[0])
            zs = ZeroShotAUROC(n_bootstrap=0, comm=self.comm)
            zs.update("val", self.predict_proba(X_val), y_val, self.classes.tolist())
            auc = zs.compute()["val"]["auc"]
            self.sweep_.append((l2, auc, self.n_iter_))
            if best is None or (auc == auc and not best[0] >= auc):          # nan never wins; strictly better only
                best = (auc, l2, self.state_dict(), (self.n_iter_, self.converged_, self.grad_norm_, self.objective_))
        _, self.l2, state, (self.n_iter_, self.converged_, self.grad_norm_, self.objective_) = best
        self.load_state_dict(state)
        return self

    def state_dict(self):
        if self.weight is None:
            raise RuntimeError("the probe is not fitted: nothing to save")
        return {"weight": self.weight.clone(), "bias": self.bias.clone(), "classes": self.classes.clone()}

    def load_state_dict(self, state):
        missing = {"weight", "bias", "classes"} - set(state)
        if missing:
            raise KeyError(f"state_dict lacks {sorted(missing)}")
        W, b, classes = state["weight"], state["bias"], state["classes"]
        if W.ndim != 2 or b.shape != (W.shape[0],) or classes.shape != (W.shape[0],):
            raise ValueError(f"weight [C,D], bias [C] and classes [C] do not agree: {tuple(W.shape)}, {tuple(b.shape)}, {tuple(classes.shape)}")
        self.weight, self.bias = W.detach().float().contiguous().clone(), b.detach().float().contiguous().clone()
        self.classes = classes.detach().to(torch.int64).cpu().clone()
        return self
