"""Restatement in numpy of the training of the reference's fully connected d-vector network (d_vector.py:168-206 nn_model.inference), for the
tests of the GPU trainer.  Test code only: the package never imports it.  UNPINNED: the reference tree holds no weights, logs or outputs of
this network and Keras is not installed; the gradients are corroborated against torch.autograd in float64 (tests/test_dnn_train_host.py).

    layer l:  z = x W_l + b_l;  a = relu(z) if relu_l;  y = a * keep / (1 - rate_l)          (inverted dropout, keep given or generated)
    loss:     log-sum-exp of the logits (row maximum subtracted) minus the label's logit; gradient (softmax - onehot) / B
    Adam:     m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  lr_t = lr sqrt(1-b2^t) / (1-b1^t);  p -= lr_t m / (sqrt(v) + 1e-7)
    plateau:  Keras 2's ReduceLROnPlateau.on_epoch_end, mode min, min_delta 1e-4, cooldown 0

The arithmetic runs in ``dtype``: float64 is the oracle, float32 the yardstick of how far single precision alone drifts."""
import numpy as np

B1, B2, EPS = 0.9, 0.999, 1e-7
LOG_HEADER = "epoch,acc,loss,lr,val_acc,val_loss"


# ---- the dropout generator, restated independently of the library's C code (include/ssp.h spells it out)
def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def dropout_keep(seed, step, layer, rows, width, rate):
    """-> bool (rows, width): True where the unit is kept"""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    k = mix32(0x9E3779B9 ^ (seed & 0xFFFFFFFF))
    for word in (seed >> 32, step & 0xFFFFFFFF, step >> 32, int(layer)):
        k = mix32(k ^ np.uint64(word))
    thr = int(float(np.float32(rate)) * 16777216.0)
    e = (np.arange(rows, dtype=np.uint64)[:, None] * 4096 + np.arange(width, dtype=np.uint64)[None, :])
    return (mix32(k ^ e) >> 8) >= thr


def glorot_uniform(rng, dims):
    """Keras' Dense defaults: kernel ~ U(-l, l), l = sqrt(6 / (fan_in + fan_out)); zero bias — drawn layer by layer from ``rng``"""
    out = []
    for d_in, units in zip(dims[:-1], dims[1:]):
        lim = np.sqrt(6.0 / (d_in + units))
        out.append((rng.uniform(-lim, lim, (d_in, units)).astype(np.float32), np.zeros(units, np.float32)))
    return out


class Net:
    """layers: list of (W (d_in, units), b (units,) or None, relu bool, rate float)"""

    def __init__(self, layers, dtype=np.float64):
        self.dtype = dtype
        self.W = [np.array(W, dtype=dtype) for W, _, _, _ in layers]
        self.b = [None if b is None else np.array(b, dtype=dtype) for _, b, _, _ in layers]
        self.relu = [bool(r) for _, _, r, _ in layers]
        self.rate = [float(np.float32(p)) for _, _, _, p in layers]
        self.mW = [np.zeros_like(W) for W in self.W]
        self.vW = [np.zeros_like(W) for W in self.W]
        self.mb = [None if b is None else np.zeros_like(b) for b in self.b]
        self.vb = [None if b is None else np.zeros_like(b) for b in self.b]
        self.t = 0
        self.dW = self.db = None
        self.keep_fn = dropout_keep     # (seed, step, layer, rows, width, rate) -> bool mask; a test may hand in the library's
        self.min_margin = np.inf        # smallest |label's logit - best other logit| any row has had: how safe the correct counts are

    @property
    def L(self):
        return len(self.W)

    def masks(self, seed, step, rows):
        return [None if self.rate[l] == 0 else self.keep_fn(seed, step, l, rows, self.W[l].shape[1], self.rate[l]) for l in range(self.L)]

    def forward(self, X, masks=None):
        """-> (inputs of every layer, outputs of every layer); masks None: dropout off"""
        dt = self.dtype
        x = np.asarray(X, dtype=dt)
        xs, ys = [], []
        for l in range(self.L):
            xs.append(x)
            z = x @ self.W[l]
            if self.b[l] is not None:
                z = z + self.b[l]
            if self.relu[l]:
                z = np.maximum(z, 0)
            if masks is not None and masks[l] is not None:
                z = np.where(masks[l], z * dt(dt(1) / (dt(1) - dt(self.rate[l]))), dt(0))
            ys.append(z)
            x = z
        return xs, ys

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

    def backward(self, xs, ys, masks, g):
        dt = self.dtype
        self.dW, self.db = [None] * self.L, [None] * self.L
        for l in range(self.L - 1, -1, -1):
            # g: gradient at layer l's OUTPUT -> at its pre-activation
            if masks is not None and masks[l] is not None:
                g = np.where(masks[l], g * dt(dt(1) / (dt(1) - dt(self.rate[l]))), dt(0))
            if self.relu[l]:
                g = np.where(ys[l] > 0, g, dt(0))
            self.dW[l] = xs[l].T @ g
            self.db[l] = None if self.b[l] is None else g.sum(axis=0)
            g = g @ self.W[l].T
        return self.dW, self.db

    def adam(self, lr):
        dt = self.dtype
        self.t += 1
        lr_t = dt(lr * np.sqrt(1.0 - B2 ** self.t) / (1.0 - B1 ** self.t))
        for P, G, M, V in ((self.W, self.dW, self.mW, self.vW), (self.b, self.db, self.mb, self.vb)):
            for l in range(self.L):
                if P[l] is None:
                    continue
                M[l][...] = dt(B1) * M[l] + dt(1 - B1) * G[l]      # (1 - beta rounded once, not the difference of roundings)
                V[l][...] = dt(B2) * V[l] + dt(1 - B2) * G[l] * G[l]
                P[l][...] = P[l] - lr_t * M[l] / (np.sqrt(V[l]) + dt(EPS))

    def step(self, X, labels, lr, seed):
        """one training step on the batch (X, labels); dropout keyed by (seed, steps taken so far) -> (loss sum, correct rows)"""
        masks = self.masks(seed, self.t, len(labels))
        xs, ys = self.forward(X, masks)
        loss, correct, g = self.loss(ys[-1], np.asarray(labels))
        self.backward(xs, ys, masks, g)
        self.adam(lr)
        return loss, correct

    def epoch(self, X, labels, order, batch_size, lr, seed):
        X, labels = np.asarray(X), np.asarray(labels)
        order = np.arange(len(labels)) if order is None else np.asarray(order)
        loss, correct = 0.0, 0
        for r0 in range(0, len(order), batch_size):
            rows = order[r0:r0 + batch_size]
            a, c = self.step(X[rows], labels[rows], lr, seed)
            loss, correct = loss + a, correct + c
        return loss, correct

    def evaluate(self, X, labels):
        _, ys = self.forward(X, None)
        loss, correct, _ = self.loss(ys[-1], np.asarray(labels))
        return loss, correct


class ReduceLROnPlateau:
    """Keras 2's callback, mode min, cooldown 0: update(val_loss, lr) -> the lr of the next epoch"""

    def __init__(self, factor=0.5, patience=2, min_lr=1e-7, min_delta=1e-4):
        self.factor, self.patience, self.min_lr, self.min_delta = factor, patience, min_lr, min_delta
        self.best, self.wait = np.inf, 0

    def update(self, val_loss, lr):
        if val_loss < self.best - self.min_delta:
            self.best, self.wait = val_loss, 0
            return lr
        self.wait += 1
        if self.wait >= self.patience and lr > self.min_lr:
            lr = max(lr * self.factor, self.min_lr)
            self.wait = 0
        return lr


def csv_rows(history):
    """the lines of Keras 2.2's CSVLogger for a history dict of lists (keys acc, loss, lr, val_acc, val_loss)"""
    rows = [LOG_HEADER]
    for e in range(len(history["loss"])):
        rows.append(",".join([str(e)] + [repr(float(history[k][e])) for k in ("acc", "loss", "lr", "val_acc", "val_loss")]))
    return rows


def fit(dims, X_train, y_train, X_val, y_val, epochs, batch_size, lr, seed, rates=(0.0, 0.0, 0.5, 0.5, 0.0), dtype=np.float64):
    """nn_model.inference as the package documents it: one numpy generator from ``seed`` draws the glorot kernels, then one permutation
    per epoch; relu after every layer but the last; the plateau schedule on val_loss -> (history, Net)"""
    rng = np.random.default_rng(seed)
    init = glorot_uniform(rng, dims)
    L = len(init)
    net = Net([(W, b, l < L - 1, rates[l]) for l, (W, b) in enumerate(init)], dtype)
    sched = ReduceLROnPlateau()
    hist = {k: [] for k in ("acc", "loss", "lr", "val_acc", "val_loss")}
    lr = float(np.float32(lr))   # (Keras keeps lr as a float32 variable: the schedule reads and writes float32 values)
    for _ in range(epochs):
        order = rng.permutation(len(y_train))
        loss, correct = net.epoch(X_train, y_train, order, batch_size, lr, seed)
        vl, vc = net.evaluate(X_val, y_val)
        for k, v in (("acc", correct / len(y_train)), ("loss", loss / len(y_train)), ("lr", lr),
                     ("val_acc", vc / len(y_val)), ("val_loss", vl / len(y_val))):
            hist[k].append(v)
        lr = float(np.float32(sched.update(vl / len(y_val), lr)))
    return hist, net
