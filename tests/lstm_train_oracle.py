"""Restatement in numpy of the training of the reference's recurrent d-vector network (d_vector.py:271-294 nn_model.inference_lstm), for the
tests of the GPU trainer.  Test code only: the package never imports it.  UNPINNED: the reference tree holds no weights, logs or outputs of
this network and Keras is not installed; the gradients are corroborated against torch.autograd in float64 and against central differences
(tests/test_lstm_train_host.py).

    cell:     z = x_t W + h_{t-1} U + b, gate blocks i | f | c | o;  i = s(z_i), f = s(z_f), g = tanh(z_c), o = s(z_o)
              c_t = f c_{t-1} + i g;  h_t = o tanh(c_t);  zero initial state;  s = hard_sigmoid clip(0.2 z + 0.5, 0, 1) or the sigmoid
    head:     logits = h_T Wd + bd
    loss:     log-sum-exp of the logits (row maximum subtracted) minus the label's logit; gradient (softmax - onehot) / B
    bptt:     for t = T-1 .. 0, dh starting as dlogits Wd^T, dc at 0:
              do = dh tanh(c_t);  dc += dh o (1 - tanh^2 c_t);  dz = [dc g s'(i) | dc c_{t-1} s'(f) | dc i (1 - g^2) | do s'(o)]
              dW += x_t^T dz;  dU += h_{t-1}^T dz;  db += sum over rows of dz;  dh = dz U^T;  dc = dc f
              s' = s (1 - s) for the sigmoid; 0.2 strictly inside (0, 1) and 0 elsewhere for hard_sigmoid
    Adam:     Keras 2's, as tests/dnn_train_oracle.py states it (eps 1e-7 outside the root)

The arithmetic runs in ``dtype``: float64 is the oracle, float32 the yardstick of how far single precision alone drifts."""
import numpy as np

from dnn_train_oracle import B1, B2, EPS, LOG_HEADER, ReduceLROnPlateau  # noqa: F401

NAMES = ("W", "U", "b", "Wd", "bd")


def keras_init(rng, d_in, units, n_class):
    """Keras' LSTM and Dense defaults drawn from ``rng`` in the order nn_model.inference_lstm documents: glorot_uniform kernel, Orthogonal
    recurrent kernel (normal matrix of the shape (units, 4 units), thin SVD, the factor of that shape), zero bias with the forget block at
    one, glorot_uniform Dense kernel, zero Dense bias -> W, U, b, Wd, bd (float32)"""
    lim = np.sqrt(6.0 / (d_in + 4 * units))
    W = rng.uniform(-lim, lim, (d_in, 4 * units)).astype(np.float32)
    a = rng.standard_normal((units, 4 * units))
    u, _, vt = np.linalg.svd(a, full_matrices=False)
    U = (u if u.shape == a.shape else vt).astype(np.float32)
    b = np.zeros(4 * units, np.float32)
    b[units:2 * units] = 1.0
    lim = np.sqrt(6.0 / (units + n_class))
    Wd = rng.uniform(-lim, lim, (units, n_class)).astype(np.float32)
    return W, U, b, Wd, np.zeros(n_class, np.float32)


class Net:
    """W (d_in, 4 units), U (units, 4 units), b (4 units,) or None, Wd (units, n_class), bd (n_class,) or None; activation 'hard_sigmoid' or
    'sigmoid'"""

    def __init__(self, W, U, b, Wd, bd, activation, dtype=np.float64):
        assert activation in ("hard_sigmoid", "sigmoid")
        self.dtype, self.activation = dtype, activation
        self.p = {"W": np.array(W, dtype=dtype), "U": np.array(U, dtype=dtype), "b": None if b is None else np.array(b, dtype=dtype).reshape(-1),
                  "Wd": np.array(Wd, dtype=dtype), "bd": None if bd is None else np.array(bd, dtype=dtype).reshape(-1)}
        self.units = self.p["U"].shape[0]
        self.m = {k: None if v is None else np.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: None if v is None else np.zeros_like(v) for k, v in self.p.items()}
        self.g = {k: None for k in NAMES}
        self.t = 0
        self.min_margin = np.inf       # smallest |label's logit - best other logit| any row has had: how safe the correct counts are
        self.min_clip = np.inf         # smallest | |z| - 2.5 | over the i, f, o pre-activations (hard_sigmoid): how safe the clip decisions are

    def _s(self, z):
        dt = self.dtype
        if self.activation == "sigmoid":
            return dt(1) / (dt(1) + np.exp(-z))
        self.min_clip = min(self.min_clip, float(np.abs(np.abs(z) - 2.5).min()))
        return np.clip(dt(0.2) * z + dt(0.5), dt(0), dt(1))

    def _ds(self, s):
        dt = self.dtype
        if self.activation == "sigmoid":
            return s * (dt(1) - s)
        return np.where((s > 0) & (s < 1), dt(0.2), dt(0))

    def forward(self, X):
        """X (B, T, d_in) -> (h_T, stash per step)"""
        dt = self.dtype
        X = np.asarray(X, dtype=dt)
        B, T, _ = X.shape
        H = self.units
        h = np.zeros((B, H), dt)
        c = np.zeros((B, H), dt)
        stash = []
        for t in range(T):
            z = X[:, t] @ self.p["W"] + h @ self.p["U"]
            if self.p["b"] is not None:
                z = z + self.p["b"]
            i, f, o = self._s(z[:, :H]), self._s(z[:, H:2 * H]), self._s(z[:, 3 * H:])
            g = np.tanh(z[:, 2 * H:3 * H])
            c_new = f * c + i * g
            h_new = o * np.tanh(c_new)
            stash.append((X[:, t], h, c, i, f, g, o, c_new))
            h, c = h_new, c_new
        return h, stash

    def logits(self, h):
        z = h @ self.p["Wd"]
        return z if self.p["bd"] is None else z + self.p["bd"]

    def loss(self, logits, labels):
        """-> (loss sum over the rows, rows whose arg-max is the label, gradient at the logits = (softmax - onehot) / B)"""
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
        return float(loss), int((np.argmax(logits, axis=1) == labels).sum()), (g / dt(len(labels))).astype(dt)

    def backward(self, h_last, stash, dlogits):
        dt = self.dtype
        p = self.p
        g = {"Wd": h_last.T @ dlogits, "bd": None if p["bd"] is None else dlogits.sum(axis=0),
             "W": np.zeros_like(p["W"]), "U": np.zeros_like(p["U"]), "b": None if p["b"] is None else np.zeros_like(p["b"])}
        dh = dlogits @ p["Wd"].T
        dc = np.zeros_like(dh)
        for x, h_prev, c_prev, i, f, gg, o, c_new in reversed(stash):
            tc = np.tanh(c_new)
            do = dh * tc
            dc = dc + dh * o * (dt(1) - tc * tc)
            dz = np.concatenate([dc * gg * self._ds(i), dc * c_prev * self._ds(f), dc * i * (dt(1) - gg * gg), do * self._ds(o)], axis=1)
            g["W"] += x.T @ dz
            g["U"] += h_prev.T @ dz
            if g["b"] is not None:
                g["b"] += dz.sum(axis=0)
            dh = dz @ p["U"].T
            dc = dc * f
        self.g = g
        return g

    def adam(self, lr):
        dt = self.dtype
        self.t += 1
        lr_t = dt(lr * np.sqrt(1.0 - B2 ** self.t) / (1.0 - B1 ** self.t))
        for k in NAMES:
            if self.p[k] is None:
                continue
            self.m[k][...] = dt(B1) * self.m[k] + dt(1 - B1) * self.g[k]
            self.v[k][...] = dt(B2) * self.v[k] + dt(1 - B2) * self.g[k] * self.g[k]
            self.p[k][...] = self.p[k] - lr_t * self.m[k] / (np.sqrt(self.v[k]) + dt(EPS))

    def step(self, X, labels, lr):
        h, stash = self.forward(X)
        loss, correct, g = self.loss(self.logits(h), np.asarray(labels))
        self.backward(h, stash, g)
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
        h, _ = self.forward(X)
        loss, correct, _ = self.loss(self.logits(h), np.asarray(labels))
        return loss, correct

    def snapshot(self):
        out = {}
        for prefix, d in (("", self.p), ("d", self.g), ("m", self.m), ("v", self.v)):
            for k in NAMES:
                out[prefix + k] = None if d[k] is None else d[k].copy()
        return out


def fit(X_train, y_train, X_val, y_val, n_class, epochs, batch_size, lr, seed, activation="hard_sigmoid", units=128, dtype=np.float64):
    """nn_model.inference_lstm as the package documents it: one numpy generator from ``seed`` draws the Keras initialisation, then one
    permutation per epoch; the plateau schedule on val_loss -> (history, Net)"""
    rng = np.random.default_rng(seed)
    net = Net(*keras_init(rng, X_train.shape[2], units, n_class), activation, dtype)
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
