"""Restatement in numpy of the training of the reference's conv + GRU d-vector network (d_vector.py:213-269 nn_model.inference_gru), for the
tests of the GPU trainer.  Test code only: the package never imports it.  UNPINNED: the reference tree holds no weights, logs or outputs of
this network and Keras is not installed; the gradients are corroborated against torch.autograd in float64 and against central differences
(tests/test_gru_train_host.py).  The forward pieces are tests/gru_oracle.py's (conv2d_same, the reset_after = False cell, l2_normalize).

    network:  Conv2D(F, (kh, kw), strides, same) -> Flatten per step -> n x GRU(return_sequences) -> mean over time -> Dense(E) ->
              y = e / n, n = sqrt(max(sum e^2, 1e-12)) -> Dense(n_class) softmax
    loss:     mean cross-entropy of the batch + 0.01 sum K^2 (the conv kernel's regularizers.l2()); a batch of B rows adds B times that
              to the loss sum; the gradient at the logits is (softmax - onehot) / B and dK gains 0.02 K
    bptt:     for t = To-1 .. 0, dh_t = the gradient from above + the recurrent part:
              da_h = dh_t (1 - z) (1 - hh^2);  da_z = dh_t (h_{t-1} - hh) s'(z);  G = da_h U_h^T;  da_r = G h_{t-1} s'(r)
              dh_{t-1} = dh_t z + G r + [da_z | da_r] [U_z | U_r]^T
              dW = x^T dA, db = column sums of dA, dU_zr = h_{t-1}^T [da_z | da_r], dU_h = (r h_{t-1})^T da_h, dx = dA W^T
              s' = s (1 - s) for the sigmoid; 0.2 strictly inside (0, 1) and 0 elsewhere for hard_sigmoid
    l2_normalize backward: dx = (dy - y (y . dy)) / n where sum e^2 >= eps, dy / n below it
    Adam:     Keras 2's, as tests/dnn_train_oracle.py states it (eps 1e-7 outside the root)

The arithmetic runs in ``dtype``: float64 is the oracle, float32 the yardstick of how far single precision alone drifts."""
import numpy as np

import gru_oracle as GO
from dnn_train_oracle import B1, B2, EPS, LOG_HEADER, ReduceLROnPlateau  # noqa: F401

LAMBDA = 0.01
L2_EPS = 1e-12


def names(n_gru):
    return ("conv_K", "conv_b") + tuple("gru%d_%s" % (i, k) for i in range(n_gru) for k in ("W", "U", "b")) + ("dense_W", "dense_b", "head_W", "head_b")


def keras_init(rng, T, D, F, units, n_gru, E, n_class, kernel=(5, 5), strides=(2, 2)):
    """Keras' defaults drawn from ``rng`` in the order nn_model.inference_gru documents -> a dict of float32 tensors: the conv kernel
    glorot_uniform (fan_in kh kw, fan_out kh kw F); per GRU layer the kernel glorot_uniform and the recurrent kernel Orthogonal over the
    shape (units, 3 units) (normal matrix, thin SVD, the factor of that shape); both Dense kernels glorot_uniform; zero biases"""
    kh, kw = kernel
    p = {"conv_K": GO.glorot(rng, (kh, kw, 1, F), kh * kw, kh * kw * F), "conv_b": np.zeros(F, np.float32)}
    d_in = -(-D // strides[1]) * F
    for i in range(n_gru):
        p["gru%d_W" % i] = GO.glorot(rng, (d_in, 3 * units), d_in, 3 * units)
        _, _, vt = np.linalg.svd(rng.standard_normal((units, 3 * units)), full_matrices=False)
        p["gru%d_U" % i] = vt.astype(np.float32)
        p["gru%d_b" % i] = np.zeros(3 * units, np.float32)
        d_in = units
    p["dense_W"], p["dense_b"] = GO.glorot(rng, (units, E), units, E), np.zeros(E, np.float32)
    p["head_W"], p["head_b"] = GO.glorot(rng, (E, n_class), E, n_class), np.zeros(n_class, np.float32)
    return p


class Net:
    """``params``: dict name -> array (a bias may be None) in Keras' layout, conv_K (kh, kw, 1, F); strides (sh, sw); activation
    'hard_sigmoid' or 'sigmoid' (the recurrent activation; reset_after = False)"""

    def __init__(self, params, strides, activation, dtype=np.float64):
        assert activation in GO.ACTIVATIONS
        self.dtype, self.activation, self.strides = dtype, activation, (int(strides[0]), int(strides[1]))
        self.n_gru = len([k for k in params if k.endswith("_U")])
        self.names = names(self.n_gru)
        self.p = {k: None if params.get(k) is None else np.array(params[k], dtype=dtype) for k in self.names}
        for k in self.names:
            if k.endswith("_b") and self.p[k] is not None:
                self.p[k] = self.p[k].reshape(-1)
        self.m = {k: None if v is None else np.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: None if v is None else np.zeros_like(v) for k, v in self.p.items()}
        self.g = {k: None for k in self.names}
        self.t = 0
        self.min_margin = np.inf       # smallest |label's logit - best other logit| any row has had: how safe the correct counts are
        self.min_clip = np.inf         # smallest | |a| - 2.5 | over the z and r pre-activations (hard_sigmoid): how safe the clip decisions are

    def _s(self, a):
        dt = self.dtype
        if self.activation == "sigmoid":
            return dt(1) / (dt(1) + np.exp(-a))
        self.min_clip = min(self.min_clip, float(np.abs(np.abs(a) - 2.5).min()))
        return np.clip(dt(0.2) * a + dt(0.5), dt(0), dt(1))

    def _ds(self, s):
        dt = self.dtype
        if self.activation == "sigmoid":
            return s * (dt(1) - s)
        return np.where((s > 0) & (s < 1), dt(0.2), dt(0))

    def _gru_forward(self, i, X):
        dt, p = self.dtype, self.p
        W, U, b = p["gru%d_W" % i], p["gru%d_U" % i], p["gru%d_b" % i]
        B, T, _ = X.shape
        H = U.shape[0]
        P = X @ W
        if b is not None:
            P = P + b
        Hs, Z, R, HH, Hp = (np.zeros((B, T, H), dt) for _ in range(5))
        h = np.zeros((B, H), dt)
        for t in range(T):
            zr = self._s(P[:, t, :2 * H] + h @ U[:, :2 * H])
            z, r = zr[:, :H], zr[:, H:]
            hh = np.tanh(P[:, t, 2 * H:] + (r * h) @ U[:, 2 * H:])
            Hp[:, t], Z[:, t], R[:, t], HH[:, t] = h, z, r, hh
            h = z * h + (dt(1) - z) * hh
            Hs[:, t] = h
        return Hs, (X, Hp, Z, R, HH)

    def forward(self, X):
        """X (B, T, D) -> (logits, stash)"""
        dt, p = self.dtype, self.p
        X = np.asarray(X, dtype=dt)
        if X.ndim == 4:
            X = X.reshape(X.shape[:3])
        h = GO.conv2d_same(X, p["conv_K"], p["conv_b"], self.strides, dt)
        layers = []
        for i in range(self.n_gru):
            h, st = self._gru_forward(i, h)
            layers.append(st)
        mean = GO.time_mean(h)
        e = mean @ p["dense_W"]
        if p["dense_b"] is not None:
            e = e + p["dense_b"]
        ss = (e * e).sum(axis=1, keepdims=True)
        n = np.sqrt(np.maximum(ss, dt(L2_EPS)))
        y = e / n
        logits = y @ p["head_W"]
        if p["head_b"] is not None:
            logits = logits + p["head_b"]
        return logits, dict(X=X, layers=layers, To=h.shape[1], mean=mean, ss=ss, n=n, y=y)

    def embedding(self, X):
        """what spkModel.predict gives: the unit-length embedding"""
        return self.forward(X)[1]["y"]

    def reg(self):
        K = self.p["conv_K"]
        return float(self.dtype(LAMBDA) * (K * K).sum(dtype=self.dtype))

    def loss(self, logits, labels):
        """-> (loss sum over the rows with the regulariser's B lambda sum K^2, rows whose arg-max is the label, gradient at the logits)"""
        dt = self.dtype
        z = logits - logits.max(axis=1, keepdims=True)
        e = np.exp(z)
        s = e.sum(axis=1, keepdims=True)
        rows = np.arange(len(labels))
        others = np.array(logits, dtype=np.float64)
        others[rows, labels] = -np.inf
        self.min_margin = min(self.min_margin, float(np.abs(logits[rows, labels] - others.max(axis=1)).min()))
        loss = (np.log(s[:, 0]) - z[rows, labels]).sum(dtype=dt)
        g = e / s
        g[rows, labels] -= 1
        return float(loss) + len(labels) * self.reg(), int((np.argmax(logits, axis=1) == labels).sum()), (g / dt(len(labels))).astype(dt)

    def backward(self, st, dlogits):
        dt, p = self.dtype, self.p
        g = {k: None for k in self.names}
        y, n, ss = st["y"], st["n"], st["ss"]
        g["head_W"] = y.T @ dlogits
        g["head_b"] = None if p["head_b"] is None else dlogits.sum(axis=0)
        dy = dlogits @ p["head_W"].T
        de = np.where(ss >= dt(L2_EPS), (dy - y * (y * dy).sum(axis=1, keepdims=True)) / n, dy / n)
        g["dense_W"] = st["mean"].T @ de
        g["dense_b"] = None if p["dense_b"] is None else de.sum(axis=0)
        dmean = de @ p["dense_W"].T
        To = st["To"]
        above = np.repeat((dmean / dt(To))[:, None, :], To, axis=1)
        for i in reversed(range(self.n_gru)):
            X, Hp, Z, R, HH = st["layers"][i]
            W, U = p["gru%d_W" % i], p["gru%d_U" % i]
            B, T, H = Z.shape
            dA = np.zeros((B, T, 3 * H), dt)
            rec = np.zeros((B, H), dt)
            for t in reversed(range(T)):
                dh = above[:, t] + rec
                z, r, hh, hp = Z[:, t], R[:, t], HH[:, t], Hp[:, t]
                da_h = dh * (dt(1) - z) * (dt(1) - hh * hh)
                da_z = dh * (hp - hh) * self._ds(z)
                G = da_h @ U[:, 2 * H:].T
                da_r = G * hp * self._ds(r)
                rec = dh * z + G * r + np.concatenate([da_z, da_r], axis=1) @ U[:, :2 * H].T
                dA[:, t, :H], dA[:, t, H:2 * H], dA[:, t, 2 * H:] = da_z, da_r, da_h
            dA2 = dA.reshape(B * T, 3 * H)
            g["gru%d_W" % i] = X.reshape(B * T, -1).T @ dA2
            g["gru%d_b" % i] = None if p["gru%d_b" % i] is None else dA2.sum(axis=0)
            Hp2 = Hp.reshape(B * T, H)
            g["gru%d_U" % i] = np.concatenate([Hp2.T @ dA2[:, :2 * H], (R.reshape(B * T, H) * Hp2).T @ dA2[:, 2 * H:]], axis=1)
            above = dA @ W.T
        # the convolution: dK and db from the gradient at its output (B, To, Do, F)
        K = p["conv_K"]
        kh, kw, _, F = K.shape
        X = st["X"]
        B, T, D = X.shape
        sh, sw = self.strides
        To, pt, pb = GO.same_padding(T, kh, sh)
        Do, pl, pr = GO.same_padding(D, kw, sw)
        dY = above.reshape(B, To, Do, F)
        Xp = np.pad(X, ((0, 0), (pt, pb), (pl, pr)))
        dK = np.zeros_like(K)
        for a in range(kh):
            for b in range(kw):
                win = Xp[:, a:a + (To - 1) * sh + 1:sh, b:b + (Do - 1) * sw + 1:sw]
                dK[a, b, 0] = np.einsum("ntf,ntfc->c", win, dY)
        g["conv_K"] = dK + dt(2 * LAMBDA) * K
        g["conv_b"] = None if p["conv_b"] is None else dY.sum(axis=(0, 1, 2))
        self.g = g
        return g

    def adam(self, lr):
        dt = self.dtype
        self.t += 1
        lr_t = dt(lr * np.sqrt(1.0 - B2 ** self.t) / (1.0 - B1 ** self.t))
        for k in self.names:
            if self.p[k] is None:
                continue
            self.m[k][...] = dt(B1) * self.m[k] + dt(1 - B1) * self.g[k]
            self.v[k][...] = dt(B2) * self.v[k] + dt(1 - B2) * self.g[k] * self.g[k]
            self.p[k][...] = self.p[k] - lr_t * self.m[k] / (np.sqrt(self.v[k]) + dt(EPS))

    def step(self, X, labels, lr):
        logits, st = self.forward(X)
        loss, correct, g = self.loss(logits, np.asarray(labels))
        self.backward(st, g)
        self.adam(lr)
        return loss, correct

    def epoch(self, X, labels, order, batch_size, lr):
        X, labels = np.asarray(X), np.asarray(labels)
        order = np.arange(len(labels)) if order is None else np.asarray(order)
        loss, correct = 0.0, 0
        for r0 in range(0, len(order), batch_size):
            rows = order[r0:r0 + batch_size]
            a, c = self.step(X[rows], labels[rows], lr)
            loss, correct = loss + a, correct + c
        return loss, correct

    def evaluate(self, X, labels):
        logits, _ = self.forward(X)
        loss, correct, _ = self.loss(logits, np.asarray(labels))
        return loss, correct

    def snapshot(self):
        out = {}
        for prefix, d in (("", self.p), ("d", self.g), ("m", self.m), ("v", self.v)):
            for k in self.names:
                out[prefix + k] = None if d[k] is None else d[k].copy()
        return out


def fit(X_train, y_train, X_val, y_val, n_class, epochs, batch_size, lr, seed, activation="hard_sigmoid", filters=64, units=1024, n_gru=3,
        embedding=512, dtype=np.float64):
    """nn_model.inference_gru as the package documents it: one numpy generator from ``seed`` draws the Keras initialisation, then one
    permutation per epoch; the plateau schedule on val_loss -> (history, Net)"""
    rng = np.random.default_rng(seed)
    T, D = X_train.shape[1], X_train.shape[2]
    net = Net(keras_init(rng, T, D, filters, units, n_gru, embedding, n_class), (2, 2), activation, dtype)
    sched = ReduceLROnPlateau()
    hist = {k: [] for k in ("acc", "loss", "lr", "val_acc", "val_loss")}
    lr = float(np.float32(lr))
    for _ in range(epochs):
        order = rng.permutation(len(y_train))
        loss, correct = net.epoch(X_train, y_train, order, batch_size, lr)
        vl, vc = net.evaluate(X_val, y_val)
        for k, v in (("acc", correct / len(y_train)), ("loss", loss / len(y_train)), ("lr", lr),
                     ("val_acc", vc / len(y_val)), ("val_loss", vl / len(y_val))):
            hist[k].append(v)
        lr = float(np.float32(sched.update(vl / len(y_val), lr)))
    return hist, net
