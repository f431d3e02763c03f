"""GPU-backed mirror of the inference half of the reference's ``d_vector.py``: Data_gen's feature front end
(d_vector.py:80-98), the forward pass of the fully connected speaker network (``DenseNet.predict`` = spkModel.predict of
the Sequential built at d_vector.py:171-189), the forward pass of the recurrent one (``LstmNet.predict``: the LSTM(128) of
d_vector.py:271-294, the network nn_model.enroll / eval load by default), the forward pass of the conv + GRU one (``ConvGruNet.predict``:
Conv2D -> 3 x GRU(1024) -> mean over time -> Dense(512) -> L2 normalisation, d_vector.py:213-269, the network d_vector.py:389 evaluates)
and nn_model.test / enroll / eval (d_vector.py:296-361), and the training of the fully connected network (``nn_model.inference``,
d_vector.py:168-210: forward with dropout, softmax cross-entropy, backward and Adam on the GPU, api.DnnTrainer) and of the recurrent one
(``nn_model.inference_lstm``, d_vector.py:271-294: recurrent forward with a stash, backward through time and Adam on the GPU,
api.LstmTrainer; it writes d_vector_lstm.npz, which enroll / eval pick up) and of the conv + GRU one (``nn_model.inference_gru``,
d_vector.py:213-269: api.GruTrainer; it writes d_vector_gru.npz, a ConvGruNet).
The recurrent networks are UNPINNED: the reference tree holds no weights or outputs for them and Keras is not a dependency; their
arithmetic is restated from Keras' documentation and corroborated against torch's cells only."""
from __future__ import annotations

import functools
import os
import pickle as pkl

import numpy as np

from . import api, frontend
from .GMM_UBM import delta as _delta


def cosine_scores(X, centroids):
    """(N, S) float64 matrix of scipy.spatial.distance.cosine(X[i], centroids[j]) — d_vector.py:315-318."""
    r = api.cosine_identify(api.default_context(), X, np.asarray(centroids, dtype=np.float32), dist=True, argmin=False, minval=False)
    return np.asarray(r["dist"], dtype=np.float64)


def identify(X, centroids, precision=0):
    """argmin_j cosine(X[i], centroids[j]) (first index on ties) — d_vector.py:319.  precision 1 / 2: the split-precision sweeps of
    ssp_cosine_identify2 (the fp32 path's index on every row through proven error bands, 3 - 5 x faster; embeddings of at most 256 dims)."""
    r = api.cosine_identify(api.default_context(), X, np.asarray(centroids, dtype=np.float32), dist=False, argmin=True, minval=False,
                            precision=int(precision))
    return np.asarray(r["argmin"]).astype(np.int64)


class DenseNet:
    """Forward pass of the reference's fully connected d-vector network (d_vector.py:171-189): Dense(256)+ReLU x 3, then
    Dense(256) — what ``load_model('feature/d_vector/d_vector_nn.h5').predict`` computes (dropout is the identity at
    inference).  ``layers``: list of (kernel (d_in, units), bias (units,) or None, activation in {'relu', 'linear', None}) in
    Keras' own layout, e.g. ``[(l.get_weights()[0], l.get_weights()[1], 'relu') ...]``.  Weights go to the GPU once."""

    def __init__(self, layers, device: int = 0):
        import torch
        self._ctx = api.default_context(device, torch_stream=True)
        self.layers = []
        d_prev = None
        for W, b, act in layers:
            W = np.asarray(W, dtype=np.float32)
            if W.ndim != 2 or (d_prev is not None and W.shape[0] != d_prev):
                raise ValueError("layer kernels must be (d_in, units) and chain")
            if act not in ('relu', 'linear', None):
                raise ValueError("activation must be 'relu' or 'linear'")
            d_prev = W.shape[1]
            Wt = torch.from_numpy(np.ascontiguousarray(W.T)).cuda(device)
            bt = None if b is None else torch.from_numpy(np.asarray(b, dtype=np.float32).reshape(-1)).cuda(device)
            self.layers.append((Wt, bt, act == 'relu'))
        self.input_dim = int(self.layers[0][0].shape[1])
        self.output_dim = int(d_prev)
        # the whole network as one packed object: hidden / output layers chained in registers (ssp_dnn)
        self._net = api.DnnForward(self._ctx, [(np.ascontiguousarray(np.asarray(W, dtype=np.float32).T),
                                                None if b is None else np.asarray(b, dtype=np.float32), act == 'relu') for W, b, act in layers])

    def predict(self, X, batch_size=None):
        """X (N, input_dim) numpy or torch CUDA tensor -> (N, output_dim) of the same kind (numpy in: float32 out).  Under
        ``with torch.cuda.stream(s)`` the copies of the numpy route run on s and the kernels on the cached context's stream:
        api.Context._ordered orders the two, here and in the other networks."""
        import torch
        is_t = api._is_torch(X)
        h = X if is_t else torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32)).cuda(self.layers[0][0].device)
        if h.ndim != 2 or h.shape[1] != self.input_dim:
            raise ValueError("X must be (N, %d)" % self.input_dim)
        h = self._net.forward(h)
        return h if is_t else h.cpu().numpy()


class LstmNet:
    """Forward pass of the reference's recurrent d-vector network (d_vector.py:271-294): one LSTM(units) over the (T, D) feature matrix
    of a chunk, the last hidden state is the embedding — what ``load_model('feature/d_vector/d_vector_lstm.h5').predict`` computes up
    to the layer the reference cuts the model at.  W (D, 4 units), U (units, 4 units), b (4 units,) or None are ``layer.get_weights()``
    as Keras stores them (gate blocks i | f | c | o).  ``recurrent_activation`` must be named: 'hard_sigmoid' (stand-alone Keras up to
    2.2, current when the reference was written) or 'sigmoid' (Keras 2.3 on, tf.keras) — the two give different embeddings and the
    weights file does not say which one trained them.  Weights go to the GPU once (api.LstmForward)."""

    def __init__(self, W, U, b=None, *, recurrent_activation, device: int = 0):
        self._ctx = api.default_context(device, torch_stream=True)
        self.W = np.ascontiguousarray(W, dtype=np.float32)
        self.U = np.ascontiguousarray(U, dtype=np.float32)
        self.b = None if b is None else np.ascontiguousarray(b, dtype=np.float32).reshape(-1)
        self.recurrent_activation = recurrent_activation
        self._net = api.LstmForward(self._ctx, self.W, self.U, self.b, recurrent_activation)
        self.input_dim = self._net.d_in
        self.output_dim = self._net.units

    @classmethod
    def from_keras(cls, layer, device: int = 0):
        """From a Keras LSTM layer (or anything with its ``get_weights()`` and ``recurrent_activation`` function)."""
        w = layer.get_weights()
        if len(w) not in (2, 3):
            raise ValueError("an LSTM layer holds [kernel, recurrent_kernel] or [kernel, recurrent_kernel, bias]")
        return cls(w[0], w[1], w[2] if len(w) == 3 else None, recurrent_activation=layer.recurrent_activation.__name__, device=device)

    def predict(self, X, batch_size=None):
        """X (N, T, D), or (N, T * D) — what nn_model.eval's reshape(1, -1) and load_data(reshape=True) hand over —, numpy or torch CUDA
        tensor -> (N, units) of the same kind (numpy in: float32 out)."""
        if not api._is_torch(X):
            X = np.asarray(X)
        if X.ndim == 2:
            if X.shape[1] == 0 or X.shape[1] % self.input_dim:
                raise ValueError("X must be (N, T, %d) or (N, T * %d)" % (self.input_dim, self.input_dim))
            X = X.reshape(X.shape[0], X.shape[1] // self.input_dim, self.input_dim)
        if X.ndim != 3 or X.shape[2] != self.input_dim:
            raise ValueError("X must be (N, T, %d) or (N, T * %d)" % (self.input_dim, self.input_dim))
        return self._net.forward(X)

    def predict_ragged(self, feats, fseg):
        """feats (frames, D) laid out by the frame segments ``fseg`` (MfccPlan.run's output, as it is) -> (n sequences, units)."""
        return self._net.forward(feats, fseg)


class ConvGruNet:
    """Forward pass of the reference's conv + GRU d-vector network (d_vector.py:213-269 inference_gru; 'feature/d_vector/d_vector_gru.h5'):
    Conv2D(F, (kh, kw), strides, padding='same') on the (T, D, 1) feature matrix of a chunk, TimeDistributed(Flatten), n GRU layers with
    return_sequences, the mean over time, Dense and K.l2_normalize.  ``conv`` = (K (kh, kw, 1, F), b (F,) or None, strides (sh, sw));
    ``grus`` = [(W (d_in, 3 units), U (units, 3 units), b or None), ...]; ``dense`` = (Wd (units, E), bd (E,) or None) — all as
    ``layer.get_weights()`` returns them.  Both GRU switches must be named, the weights do not record them: ``recurrent_activation``
    'hard_sigmoid' (stand-alone Keras up to 2.2) or 'sigmoid', ``reset_after`` False (stand-alone Keras, bias (3 units,)) or True (tf.keras 2,
    bias (2, 3 units)).  ``input_shape`` = (T, D) lets predict take flattened (N, T * D) rows.  A batch runs in slabs of chunks whose
    intermediate activations fit ``workspace_bytes`` (default 4 GiB); a chunk's embedding does not depend on the slab it is in.  Layers
    chain on the device.  Unpinned against Keras (no GRU fixture in the reference, no Keras here): corroborated against torch only."""

    DEFAULT_WORKSPACE = 4 << 30

    def __init__(self, conv, grus, dense, *, recurrent_activation, reset_after, input_shape=None, workspace_bytes=None, device: int = 0):
        if recurrent_activation not in api.GRU_ACTIVATIONS:
            raise ValueError("recurrent_activation must be 'hard_sigmoid' or 'sigmoid'")
        if not isinstance(reset_after, (bool, np.bool_)):
            raise ValueError("reset_after must be True or False")
        K, bc, strides = conv
        self.K = np.ascontiguousarray(K, dtype=np.float32)
        if self.K.ndim == 3:
            self.K = self.K[:, :, None, :]
        if self.K.ndim != 4 or self.K.shape[2] != 1:
            raise ValueError("the convolution kernel must be (kh, kw, 1, F)")
        self.bc = None if bc is None else np.ascontiguousarray(bc, dtype=np.float32).reshape(-1)
        self.strides = (int(strides[0]), int(strides[1]))
        if len(grus) < 1:
            raise ValueError("at least one GRU layer")
        self.grus = [api._gru_arrays(W, U, b, reset_after) for W, U, b in grus]
        Wd, bd = dense
        self.Wd = np.ascontiguousarray(Wd, dtype=np.float32)
        self.bd = None if bd is None else np.ascontiguousarray(bd, dtype=np.float32).reshape(-1)
        F = int(self.K.shape[3])
        for i, (W, U, _) in enumerate(self.grus):
            if i and W.shape[0] != self.grus[i - 1][1].shape[0]:
                raise ValueError("GRU layer %d does not take layer %d's width" % (i, i - 1))
        if self.grus[0][0].shape[0] % F:
            raise ValueError("the first GRU's input width must be a multiple of the %d filters" % F)
        if self.Wd.ndim != 2 or self.Wd.shape[0] != self.grus[-1][1].shape[0]:
            raise ValueError("the Dense kernel must be (units, E)")
        self.recurrent_activation, self.reset_after = recurrent_activation, bool(reset_after)
        self.input_shape = None if input_shape is None else (int(input_shape[0]), int(input_shape[1]))
        self.workspace_bytes = int(self.DEFAULT_WORKSPACE if workspace_bytes is None else workspace_bytes)
        if self.workspace_bytes < 1:
            raise ValueError("workspace_bytes must be positive")
        self.output_dim = int(self.Wd.shape[1])
        import torch
        self._ctx = api.default_context(device, torch_stream=True)
        self._dev = "cuda:%d" % device
        self._K = torch.from_numpy(self.K).to(self._dev)
        self._bc = None if self.bc is None else torch.from_numpy(self.bc).to(self._dev)
        self._layers = [api.GruForward(self._ctx, W, U, b, recurrent_activation, bool(reset_after)) for W, U, b in self.grus]
        self._Wdt = torch.from_numpy(np.ascontiguousarray(self.Wd.T)).to(self._dev)
        self._bd = None if self.bd is None else torch.from_numpy(self.bd).to(self._dev)
        self.last_slab = 0

    @classmethod
    def from_keras(cls, model, *, recurrent_activation, reset_after, input_shape=None, workspace_bytes=None, device: int = 0):
        """From a Keras model (or anything whose ``layers`` have ``get_weights()``): the layers that hold weights are taken in order — one
        Conv2D (4-D kernel; ``strides`` read from the layer), the GRUs (two 2-D kernels) and the Dense (one 2-D kernel)."""
        conv, grus, dense = None, [], None
        for layer in model.layers:
            w = layer.get_weights()
            if not w:
                continue
            if np.ndim(w[0]) == 4:
                conv = (w[0], w[1] if len(w) > 1 else None, tuple(getattr(layer, "strides", (1, 1))))
            elif len(w) >= 2 and np.ndim(w[1]) == 2:
                grus.append((w[0], w[1], w[2] if len(w) > 2 else None))
            else:
                dense = (w[0], w[1] if len(w) > 1 else None)
        if conv is None or not grus or dense is None:
            raise ValueError("expected a Conv2D, GRU layers and a Dense among the model's layers")
        return cls(conv, grus, dense, recurrent_activation=recurrent_activation, reset_after=reset_after, input_shape=input_shape,
                   workspace_bytes=workspace_bytes, device=device)

    def _slab(self, T, D):
        To, Do = api.conv2d_same_out_shape(T, D, self.strides)
        F = int(self.K.shape[3])
        if Do * F != self.grus[0][0].shape[0]:
            raise ValueError("a (%d, %d) input gives %d features per step, the first GRU takes %d" % (T, D, Do * F, self.grus[0][0].shape[0]))
        widths = [U.shape[0] for _, U, _ in self.grus]
        seq = sorted(widths, reverse=True)[:2]     # two sequences are alive at a time (a layer's input and its output)
        per = 4 * To * (Do * F + sum(seq) + 3 * max(widths)) + 4 * 2 * max(widths)
        return max(1, self.workspace_bytes // per), per, To

    def predict(self, X, batch_size=None, parts=None):
        """X (N, T, D, 1) or (N, T, D) — or (N, T * D) when ``input_shape`` was given —, numpy or torch CUDA tensor -> (N, E) unit-length
        embeddings of the same kind (numpy in: float32 out).  ``parts``: a dict that receives 'mean' (the last GRU's mean over time) and,
        with a 'ms' key present, the kernel milliseconds of each stage summed over the slabs (each reading synchronises)."""
        import torch
        is_t = api._is_torch(X)
        if not is_t:
            X = np.asarray(X)
        if X.ndim == 2 and self.input_shape is not None and X.shape[1] == self.input_shape[0] * self.input_shape[1]:
            X = X.reshape(X.shape[0], self.input_shape[0], self.input_shape[1])
        if X.ndim == 4 and X.shape[3] == 1:
            X = X.reshape(X.shape[0], X.shape[1], X.shape[2])
        if X.ndim != 3 or X.shape[1] < 1 or X.shape[2] < 1:
            raise ValueError("X must be (N, T, D, 1) or (N, T, D)" + ("" if self.input_shape is None else " or (N, %d)" % (self.input_shape[0] * self.input_shape[1])))
        N, T, D = (int(v) for v in X.shape)
        slab, _, _ = self._slab(T, D)
        self.last_slab = min(slab, N)
        out = torch.empty((N, self.output_dim), dtype=torch.float32, device=self._dev)
        H = int(self.grus[-1][1].shape[0])
        mean_all = torch.empty((N, H), dtype=torch.float32, device=self._dev) if parts is not None else None
        timing = parts is not None and "ms" in parts
        ms = {"conv": 0.0, "gru": [0.0] * len(self._layers), "tail": 0.0}
        for c0 in range(0, N, slab):
            x = X[c0:c0 + slab]
            if not is_t:
                x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self._dev)
            r = api.conv2d_same(self._ctx, x, self._K, self._bc, self.strides, timing=timing)
            h, t_ms = r if timing else (r, 0.0)
            ms["conv"] += t_ms
            for i, g in enumerate(self._layers):
                g.set_workspace(self.workspace_bytes)
                r = g.forward(h, mean=i == len(self._layers) - 1, timing=timing)
                h, t_ms = r if timing else (r, 0.0)
                ms["gru"][i] += t_ms
            if mean_all is not None:
                mean_all[c0:c0 + slab] = h
            r = api.dense_forward(self._ctx, h, self._Wdt, self._bd, relu=False, timing=timing)
            y, t_ms = r if timing else (r, 0.0)
            ms["tail"] += t_ms
            r = api.l2_normalize(self._ctx, y, timing=timing)
            y, t_ms = r if timing else (r, 0.0)
            ms["tail"] += t_ms
            out[c0:c0 + slab] = y
        if parts is not None:
            parts["mean"] = mean_all if is_t else mean_all.cpu().numpy()
            if timing:
                parts["ms"] = ms
        return out if is_t else out.cpu().numpy()


# ---- model registry: the reference addresses its networks by name — load_model('feature/d_vector/d_vector_{}.h5'.format(model_name)),
# d_vector.py:297,329,347.  Keras / h5py are not part of this path: a DenseNet is registered under the name (or saved next to where
# the .h5 would be, as d_vector_{name}.npz) and `model_name=` resolves to it.
_MODELS = {}
MODEL_DIR = os.path.join('feature', 'd_vector')


def register_model(name, net):
    """Make ``net`` (a DenseNet, an LstmNet, a ConvGruNet, or any object with .predict) the model that ``model_name=name`` refers to."""
    _MODELS[str(name)] = net


def save_model(net, name, model_dir=None):
    """Store a DenseNet's, an LstmNet's or a ConvGruNet's weights as {model_dir}/d_vector_{name}.npz (the .h5's place, d_vector.py:297).
    An LstmNet's file carries kind = 'lstm' and its recurrent activation, a ConvGruNet's kind = 'conv_gru' with both GRU switches, the
    strides and the input shape; a file without ``kind`` is a DenseNet."""
    model_dir = MODEL_DIR if model_dir is None else model_dir
    os.makedirs(model_dir, exist_ok=True)
    if isinstance(net, ConvGruNet):
        arrs = {"kind": np.array("conv_gru"), "recurrent_activation": np.array(net.recurrent_activation), "reset_after": np.array(int(net.reset_after)),
                "strides": np.array(net.strides, np.int64), "n_gru": np.array(len(net.grus)), "conv_K": net.K,
                "conv_b": np.zeros(0, np.float32) if net.bc is None else net.bc, "dense_W": net.Wd,
                "dense_b": np.zeros(0, np.float32) if net.bd is None else net.bd,
                "input_shape": np.array(net.input_shape if net.input_shape is not None else (), np.int64)}
        for i, (W, U, b) in enumerate(net.grus):
            arrs["gru%d_W" % i], arrs["gru%d_U" % i], arrs["gru%d_b" % i] = W, U, np.zeros(0, np.float32) if b is None else b
        np.savez(os.path.join(model_dir, "d_vector_%s.npz" % name), **arrs)
        return
    if isinstance(net, LstmNet):
        np.savez(os.path.join(model_dir, "d_vector_%s.npz" % name), kind=np.array("lstm"), W=net.W, U=net.U,
                 b=np.zeros(0, np.float32) if net.b is None else net.b, recurrent_activation=np.array(net.recurrent_activation))
        return
    arrs = {}
    for i, (Wt, bt, relu) in enumerate(net.layers):
        arrs["W%d" % i] = Wt.cpu().numpy().T
        arrs["b%d" % i] = np.zeros(0, np.float32) if bt is None else bt.cpu().numpy()
        arrs["a%d" % i] = np.array(1 if relu else 0)
    np.savez(os.path.join(model_dir, "d_vector_%s.npz" % name), **arrs)


def load_model(name, model_dir=None):
    """The network ``model_name`` refers to: a registered one, else {model_dir}/d_vector_{name}.npz; OSError when neither exists (as
    keras.models.load_model raises for a missing file)."""
    name = str(name)
    if name in _MODELS:
        return _MODELS[name]
    path = os.path.join(MODEL_DIR if model_dir is None else model_dir, "d_vector_%s.npz" % name)
    if not os.path.exists(path):
        raise OSError("no d-vector model %r: register_model(%r, net) or save one as %s" % (name, name, path))
    z = np.load(path)
    if "kind" in z.files:
        if str(z["kind"]) == "conv_gru":
            opt = lambda a: a if a.size else None  # noqa: E731
            net = ConvGruNet((z["conv_K"], opt(z["conv_b"]), tuple(int(v) for v in z["strides"])),
                             [(z["gru%d_W" % i], z["gru%d_U" % i], opt(z["gru%d_b" % i])) for i in range(int(z["n_gru"]))],
                             (z["dense_W"], opt(z["dense_b"])), recurrent_activation=str(z["recurrent_activation"]),
                             reset_after=bool(int(z["reset_after"])), input_shape=tuple(int(v) for v in z["input_shape"]) if z["input_shape"].size else None)
            _MODELS[name] = net
            return net
        if str(z["kind"]) != "lstm":
            raise ValueError("%s: unknown model kind %r" % (path, str(z["kind"])))
        net = LstmNet(z["W"], z["U"], z["b"] if z["b"].size else None, recurrent_activation=str(z["recurrent_activation"]))
        _MODELS[name] = net
        return net
    n = len([k for k in z.files if k.startswith("W")])
    net = DenseNet([(z["W%d" % i], z["b%d" % i] if z["b%d" % i].size else None, 'relu' if int(z["a%d" % i]) else 'linear') for i in range(n)])
    _MODELS[name] = net
    return net


_UNSET = object()


def _resolve_model(model_name, spk_model, default_name):
    """spk_model= (an object) wins; an explicit model_name= must resolve (OSError otherwise, like the reference); with neither given the
    reference's default name is tried and, when no such model exists, the inputs are taken to be embeddings already."""
    if spk_model is not None:
        return spk_model
    if model_name is _UNSET:
        try:
            return load_model(default_name)
        except OSError:
            return None
    if model_name is None:
        return None
    return model_name if hasattr(model_name, "predict") else load_model(model_name)


@functools.lru_cache(maxsize=8)
def _feature_plan(feature_type, sample_rate):
    if feature_type == 'PLP':  # d_vector.py:92-93: plp(x, fs)[0]
        return api.MfccPlan(api.default_context(), frontend.preset_sidekit_plp(fs=sample_rate))
    if feature_type != 'MFCC':
        raise NameError  # d_vector.py:94-95
    return api.MfccPlan(api.default_context(), frontend.preset_sidekit(fs=sample_rate))


class Data_gen:
    """Feature front end of d_vector.Data_gen: 1-second chunks -> sidekit mfcc(x, fs)[0] -> (98, 13) (d_vector.py:80-98)."""

    def __init__(self, sample_rate=16000):
        self.sample_rate = sample_rate
        self.path = None  # the dataset directory of _load() (the reference's load_data sets it)

    @staticmethod
    def delta(feat, N=2):
        """d_vector.py:143-160 (identical to GMM_UBM.delta)."""
        return _delta(feat, N)

    def _plan(self, feature_type):
        return _feature_plan(feature_type, int(self.sample_rate))  # (keyed on the rate too: _load() takes it from the files)

    def _load(self):
        """d_vector.py:34-57 — every wav under ``self.path/<speaker>/<dir>/``: (list of audio arrays, list of speaker names); the sample
        rate of the files becomes ``self.sample_rate``."""
        from .utils.tools import read
        x, y = [], []
        for speaker in os.listdir(self.path):
            path1 = os.path.join(self.path, speaker)
            for _dir in os.listdir(path1):
                path2 = os.path.join(path1, _dir)
                for _wav in os.listdir(path2):
                    self.sample_rate, audio = read(os.path.join(path2, _wav))
                    y.append(speaker)
                    x.append(audio)
        return x, y

    @staticmethod
    def save(data, file_name):
        """d_vector.py:133-136"""
        with open('feature/{}.pkl'.format(file_name), 'wb') as f:
            pkl.dump(data, f)

    @staticmethod
    def load(file_name):
        """d_vector.py:138-141"""
        with open('feature/{}.pkl'.format(file_name), 'rb') as f:
            return pkl.load(f)

    def extract_feature(self, *args, feature_type='MFCC', datatype='dev'):
        """Two call shapes.  The reference's (d_vector.py:59-118): ``extract_feature(feature_type='MFCC', datatype='dev')`` — audio from
        ``self._load()`` (``self.path`` set by the caller, as ``load_data`` does), features cached under ``feature/<datatype>_<type>_*.pkl``
        exactly as the reference caches them.  And the in-memory one: ``extract_feature(x, y, feature_type='MFCC')`` with x a list of audio
        arrays and y their labels.  Either way every audio is cut into 1 s chunks (d_vector.py:80-83), all chunks go through ONE kernel
        launch, and chunks whose features contain NaN are dropped (d_vector.py:97-98).  Returns (feature, label)."""
        if args and not isinstance(args[0], str):
            if len(args) < 2 or len(args) > 3:
                raise TypeError("extract_feature(x, y, feature_type='MFCC') or extract_feature(feature_type='MFCC', datatype='dev')")
            if len(args) == 3:
                feature_type = args[2]
            return self._extract(args[0], args[1], feature_type)
        if len(args) > 2:
            raise TypeError("extract_feature(feature_type='MFCC', datatype='dev')")
        if len(args) >= 1:
            feature_type = args[0]
        if len(args) == 2:
            datatype = args[1]
        if not os.path.exists('feature'):
            os.mkdir('feature')
        if os.path.exists('feature/{}_{}_feature.pkl'.format(datatype, feature_type)):
            return self.load('{}_{}_feature'.format(datatype, feature_type)), self.load('{}_{}_label'.format(datatype, feature_type))
        x, y = self._load()
        feature, label = self._extract(x, y, feature_type)
        self.save(feature, '{}_{}_feature'.format(datatype, feature_type))
        self.save(label, '{}_{}_label'.format(datatype, feature_type))
        return feature, label

    def _extract(self, x, y, feature_type='MFCC'):
        # ('MFCC_PLP', UI/tmp.py:319-324: hstack(mfcc, plp) per chunk, runs both front ends through sidekit_features.plp_features_batch)
        plan = None if feature_type == 'MFCC_PLP' else self._plan(feature_type)
        sr = self.sample_rate
        chunks, labels = [], []
        for xi, yi in zip(x, y):
            xi = np.asarray(xi).reshape(-1)   # (int16 PCM stays int16: api.flatten_signals below)
            for j in range(xi.shape[0] // sr):
                chunks.append(xi[j * sr:(j + 1) * sr])
                labels.append(yi)
        if not chunks:
            return [], []
        if plan is None:
            from .sidekit_features import plp_features_batch
            feats, fseg = plp_features_batch(chunks, fs=int(sr), with_mfcc=True)
        else:
            seg = api.Segments.from_lengths(plan.ctx, [sr] * len(chunks))
            fseg = plan.frame_segments(seg)
            feats = plan.run(api.flatten_signals(chunks)[0], seg, fseg)
            if feature_type == 'PLP':
                feats = api.plp_post(plan.ctx, feats, fseg, sr / 2.0)
        feats = np.asarray(feats, dtype=np.float64)
        feature, label = [], []
        for i, lab in enumerate(labels):
            f = feats[fseg.offsets[i]:fseg.offsets[i + 1]]
            if np.isnan(f).sum() > 0:
                continue
            feature.append(f)
            label.append(lab)
        return feature, label


class nn_model:
    """d_vector.nn_model: ``inference`` trains the fully connected network, ``inference_lstm`` the recurrent one and ``inference_gru`` the conv +
    GRU one (reset_after=False, stand-alone Keras' cell, only); test / enroll / eval score.  ``X_*`` are embeddings, or network inputs when ``spk_model`` (a DenseNet, the
    stand-in for load_model('feature/d_vector/d_vector_{}.h5')) is given.  ``store``: path of the enrolment dictionary pickle
    (the reference always uses 'feature/d_vector/d_vector.pkl', d_vector.py:333-344,350-351); None keeps it in memory."""

    def __init__(self, n_class=40, store=None):
        # (n_class: the reference's only constructor argument, d_vector.py:165 — the width of the training network's softmax; the inference
        #  half kept here never reads it, but nn_model(n_class=40) and nn_model(40) must construct)
        if isinstance(n_class, (str, os.PathLike)) and store is None:  # (round 4's signature: nn_model('path.pkl'))
            n_class, store = 40, n_class
        self.n_class = n_class
        self.store = store
        self.d_vector = {}  # name -> mean embedding, the dict the reference pickles (d_vector.py:333-344)

    def _load(self):
        if self.store is not None:
            try:
                with open(self.store, 'rb') as f:
                    self.d_vector = pkl.load(f)
            except Exception:  # d_vector.py:336-337: a missing / unreadable file starts an empty dictionary
                self.d_vector = {}

    def _save(self):
        if self.store is not None:
            d = os.path.dirname(self.store)
            if d and not os.path.exists(d):
                os.makedirs(d)
            with open(self.store, 'wb') as f:
                pkl.dump(self.d_vector, f)

    #: dropout after each of the five Dense layers (d_vector.py:175, 179, 183, 192; none behind the softmax layer)
    DROPOUT = (0.0, 0.0, 0.5, 0.5, 0.0)
    LOG_HEADER = "epoch,acc,loss,lr,val_acc,val_loss"  # Keras 2.2's CSVLogger columns, in its sorted order

    def _fit(self, net, xt, yt, xv, yv, rng, epochs, batch_size, lr, log_path, **epoch_args):
        """spk.fit's loop around a trainer (api.DnnTrainer / api.LstmTrainer / api.GruTrainer): one permutation of the rows from ``rng`` and one
        ``net.epoch`` per epoch, the validation pass, one CSVLogger row in ``log_path`` and Keras 2's ReduceLROnPlateau(val_loss, factor
        0.5, patience 2, min_lr 1e-7, min_delta 1e-4, mode min, cooldown 0) on the host -> the history as a dict of lists"""
        n_train, n_val = int(yt.shape[0]), int(yv.shape[0])
        hist = {k: [] for k in ("acc", "loss", "lr", "val_acc", "val_loss")}
        lr = float(np.float32(lr))   # (Keras keeps lr in a float32 variable)
        best, wait, factor, patience, min_lr, min_delta = np.inf, 0, 0.5, 2, 1e-7, 1e-4
        os.makedirs(os.path.dirname(log_path) or ".", exist_ok=True)
        with open(log_path, "w") as log:
            log.write(self.LOG_HEADER + "\n")
            for epoch in range(int(epochs)):
                order = rng.permutation(n_train)
                loss, correct = net.epoch(xt, yt, order, batch_size=batch_size, lr=lr, **epoch_args)
                vloss, vcorrect = net.evaluate(xv, yv) if n_val else (float("nan"), 0)
                row = {"acc": correct / max(n_train, 1), "loss": loss / max(n_train, 1), "lr": lr,
                       "val_acc": vcorrect / max(n_val, 1), "val_loss": vloss / max(n_val, 1)}
                for k, v in row.items():
                    hist[k].append(v)
                log.write(",".join([str(epoch)] + [repr(float(row[k])) for k in ("acc", "loss", "lr", "val_acc", "val_loss")]) + "\n")
                log.flush()
                # ReduceLROnPlateau.on_epoch_end (Keras 2, mode min, cooldown 0)
                if row["val_loss"] < best - min_delta:
                    best, wait = row["val_loss"], 0
                else:
                    wait += 1
                    if wait >= patience and lr > min_lr:
                        lr = float(np.float32(max(lr * factor, min_lr)))
                        wait = 0
        return hist

    def inference(self, X_train, Y_train, X_val, Y_val, *, epochs=50, batch_size=128, lr=1e-4, seed=0, model_dir=None):
        """d_vector.py:168-210, same positional signature: train Dense(256) ReLU x 3, Dense(256) | ReLU Dropout(0.5) Dense(n_class)
        softmax with categorical cross-entropy and Adam on the GPU (api.DnnTrainer), ReduceLROnPlateau(val_loss, factor 0.5, patience 2,
        min_lr 1e-7, Keras 2's min_delta 1e-4) on the host, one row per epoch in {model_dir}/nn_training.log, and the first four layers
        (spkModel) saved as {model_dir}/d_vector_nn.npz and registered under 'nn'.  One numpy generator seeded with ``seed`` draws the
        glorot_uniform kernels (zero biases: Keras' Dense defaults) layer by layer and then one permutation of the rows per epoch; the
        same ``seed`` keys the dropout.  One-hot Y is decoded with argmax.  The defaults are the reference's.  Returns the history as a
        dict of lists (acc, loss, lr, val_acc, val_loss; ``loss`` / ``acc`` are the means over the epoch's steps as they ran,
        ``val_*`` a pass without dropout after it, ``lr`` what the epoch ran with)."""
        print("Training model")
        model_dir = MODEL_DIR if model_dir is None else model_dir
        X_train, X_val = np.ascontiguousarray(X_train, dtype=np.float32), np.ascontiguousarray(X_val, dtype=np.float32)
        y_train, y_val = (np.argmax(np.asarray(Y), axis=1).astype(np.int32) for Y in (Y_train, Y_val))
        if X_train.ndim != 2 or X_val.ndim != 2 or X_val.shape[1] != X_train.shape[1] or len(y_train) != len(X_train) or len(y_val) != len(X_val):
            raise ValueError("X (N, d) and one-hot Y (N, n_class) must agree")
        if max(int(y_train.max(initial=0)), int(y_val.max(initial=0))) >= int(self.n_class):
            raise ValueError("a label lies outside n_class = %d" % self.n_class)
        dims = [int(X_train.shape[1]), 256, 256, 256, 256, int(self.n_class)]
        rng = np.random.default_rng(seed)
        layers = []
        for l, (d_in, units) in enumerate(zip(dims[:-1], dims[1:])):
            lim = np.sqrt(6.0 / (d_in + units))
            layers.append((rng.uniform(-lim, lim, (d_in, units)).astype(np.float32), np.zeros(units, np.float32), l < len(dims) - 2, self.DROPOUT[l]))
        import torch
        ctx = api.default_context()
        net = api.DnnTrainer(ctx, layers, max_batch=max(1, min(1024, max(int(batch_size), 256))))
        dev = "cuda:%d" % ctx.device
        xt, yt = torch.from_numpy(X_train).to(dev), torch.from_numpy(y_train).to(dev)   # the data stays on the device over the epochs
        xv, yv = torch.from_numpy(X_val).to(dev), torch.from_numpy(y_val).to(dev)
        hist = self._fit(net, xt, yt, xv, yv, rng, epochs, batch_size, lr, os.path.join(model_dir, "nn_training.log"), seed=seed)
        spk = DenseNet([(net.read("W", l), net.read("b", l), 'relu' if l < 3 else 'linear') for l in range(4)], device=ctx.device)
        save_model(spk, 'nn', model_dir)
        register_model('nn', spk)
        self.trainer_ = net
        return hist

    def inference_lstm(self, X_train, Y_train, X_val, Y_val, *, epochs=50, batch_size=128, lr=1e-4, seed=0, recurrent_activation='hard_sigmoid',
                       D=None, model_dir=None):
        """d_vector.py:271-294, same positional signature: train LSTM(128) -> Dense(n_class) softmax with categorical cross-entropy and Adam
        on the GPU (api.LstmTrainer: recurrent forward with a stash, backward through time, weight gradients and Adam as kernels), the
        plateau schedule and one row per epoch in {model_dir}/lstm_training.log (d_vector.py:286-287) on the host, and the LSTM alone
        (spkModel, d_vector.py:277) saved as {model_dir}/d_vector_lstm.npz and registered under 'lstm' — the model ``enroll`` and ``eval``
        load by default.  X is (N, T, D), or (N, T * D) with ``D`` given, as LstmNet.predict accepts.  ``recurrent_activation`` defaults to
        Keras <= 2.2's 'hard_sigmoid' (the Keras whose Adam(lr=) and CSVLogger columns ``inference`` follows); the saved file records it, so
        training and prediction agree.  Initialisation is Keras' own, drawn from one ``np.random.default_rng(seed)`` in this order: the LSTM
        kernel glorot_uniform over (D, 512); the recurrent kernel Orthogonal over the shape (128, 512) — a standard normal matrix of that
        shape, its thin SVD, the factor of that shape: orthonormal rows —; zero bias with the forget block at one (unit_forget_bias); the
        Dense kernel glorot_uniform with zero bias; then one permutation of the rows per epoch.  Returns the history as ``inference``
        does and keeps ``self.trainer_``.  Unpinned against Keras (no Keras here, no fixture in the reference)."""
        print("Training model")
        if recurrent_activation not in api.LSTM_ACTIVATIONS:
            raise ValueError("recurrent_activation must be 'hard_sigmoid' or 'sigmoid'")
        model_dir = MODEL_DIR if model_dir is None else model_dir
        X_train, X_val = np.ascontiguousarray(X_train, dtype=np.float32), np.ascontiguousarray(X_val, dtype=np.float32)
        if X_train.ndim == 2 and D is not None and X_train.shape[1] % int(D) == 0 and X_train.shape[1] > 0:
            X_train = X_train.reshape(X_train.shape[0], -1, int(D))
        if X_train.ndim != 3:
            raise ValueError("X must be (N, T, D), or (N, T * D) with D given")
        T, d_in = int(X_train.shape[1]), int(X_train.shape[2])
        if X_val.ndim == 2 and X_val.shape[1] == T * d_in:
            X_val = X_val.reshape(X_val.shape[0], T, d_in)
        y_train, y_val = (np.argmax(np.asarray(Y), axis=1).astype(np.int32) for Y in (Y_train, Y_val))
        if X_val.shape[1:] != X_train.shape[1:] or len(y_train) != len(X_train) or len(y_val) != len(X_val):
            raise ValueError("X (N, T, D) and one-hot Y (N, n_class) must agree")
        if max(int(y_train.max(initial=0)), int(y_val.max(initial=0))) >= int(self.n_class):
            raise ValueError("a label lies outside n_class = %d" % self.n_class)
        units, n_class = 128, int(self.n_class)
        rng = np.random.default_rng(seed)
        lim = np.sqrt(6.0 / (d_in + 4 * units))
        W = rng.uniform(-lim, lim, (d_in, 4 * units)).astype(np.float32)
        _, _, vt = np.linalg.svd(rng.standard_normal((units, 4 * units)), full_matrices=False)
        U = vt.astype(np.float32)
        b = np.zeros(4 * units, np.float32)
        b[units:2 * units] = 1.0
        lim = np.sqrt(6.0 / (units + n_class))
        Wd = rng.uniform(-lim, lim, (units, n_class)).astype(np.float32)
        bd = np.zeros(n_class, np.float32)
        import torch
        ctx = api.default_context()
        net = api.LstmTrainer(ctx, W, U, b, Wd, bd, T=T, recurrent_activation=recurrent_activation,
                              max_batch=max(1, min(1024, max(int(batch_size), 128))))
        dev = "cuda:%d" % ctx.device
        xt, yt = torch.from_numpy(X_train).to(dev), torch.from_numpy(y_train).to(dev)   # the data stays on the device over the epochs
        xv, yv = torch.from_numpy(X_val).to(dev), torch.from_numpy(y_val).to(dev)
        hist = self._fit(net, xt, yt, xv, yv, rng, epochs, batch_size, lr, os.path.join(model_dir, "lstm_training.log"))
        spk = LstmNet(net.read("W"), net.read("U"), net.read("b"), recurrent_activation=recurrent_activation, device=ctx.device)
        save_model(spk, 'lstm', model_dir)
        register_model('lstm', spk)
        self.trainer_ = net
        return hist

    def inference_gru(self, X_train, Y_train, X_val, Y_val, *, epochs=50, batch_size=128, lr=1e-4, seed=0, recurrent_activation='hard_sigmoid',
                      reset_after=False, filters=64, units=1024, n_gru=3, embedding=512, model_dir=None):
        """d_vector.py:213-269, same positional signature: train Conv2D(filters, 5 x 5, strides 2, same, l2-regularised kernel) ->
        TimeDistributed(Flatten) -> n_gru x GRU(units, return_sequences) -> mean over time -> Dense(embedding) -> l2_normalize ->
        Dense(n_class) softmax with categorical cross-entropy and Adam on the GPU (api.GruTrainer), the plateau schedule and one row per
        epoch in {model_dir}/gru_training.log on the host.  spkModel — everything up to the L2 normalisation, d_vector.py:250 — is saved as
        a ConvGruNet in {model_dir}/d_vector_gru.npz and registered under 'gru'.  X is (N, T, D, 1) or (N, T, D).  ``loss`` / ``val_loss``
        contain the regulariser's 0.01 sum K^2 as Keras reports them.  ``reset_after=True`` (tf.keras 2's cell) is not trained:
        NotImplementedError.  Initialisation is Keras' own, drawn from one ``np.random.default_rng(seed)`` in this order: the conv kernel
        glorot_uniform with fan_in kh kw and fan_out kh kw filters; then per GRU layer its kernel glorot_uniform over (d_in, 3 units) and
        its recurrent kernel Orthogonal over the shape (units, 3 units) — a standard normal matrix of that shape, its thin SVD, the
        factor of that shape: orthonormal rows, as inference_lstm draws its own —; the Dense(embedding) kernel and the head's kernel
        glorot_uniform; every bias zero; then one permutation of the rows per epoch.  Returns the history as ``inference`` does and
        keeps ``self.trainer_``.  Unpinned against Keras (no Keras here, no fixture in the reference)."""
        print("Training model")
        if recurrent_activation not in api.GRU_ACTIVATIONS:
            raise ValueError("recurrent_activation must be 'hard_sigmoid' or 'sigmoid'")
        if reset_after:
            raise NotImplementedError("inference_gru trains the reset_after=False cell only (ConvGruNet predicts with either)")
        model_dir = MODEL_DIR if model_dir is None else model_dir
        X_train, X_val = np.ascontiguousarray(X_train, dtype=np.float32), np.ascontiguousarray(X_val, dtype=np.float32)
        if X_train.ndim == 4 and X_train.shape[3] == 1:
            X_train = X_train.reshape(X_train.shape[:3])
        if X_val.ndim == 4 and X_val.shape[3] == 1:
            X_val = X_val.reshape(X_val.shape[:3])
        y_train, y_val = (np.argmax(np.asarray(Y), axis=1).astype(np.int32) for Y in (Y_train, Y_val))
        if X_train.ndim != 3 or X_val.shape[1:] != X_train.shape[1:] or len(y_train) != len(X_train) or len(y_val) != len(X_val):
            raise ValueError("X (N, T, D[, 1]) and one-hot Y (N, n_class) must agree")
        if max(int(y_train.max(initial=0)), int(y_val.max(initial=0))) >= int(self.n_class):
            raise ValueError("a label lies outside n_class = %d" % self.n_class)
        T, D = int(X_train.shape[1]), int(X_train.shape[2])
        kh, kw, strides = 5, 5, (2, 2)
        F, H, E, n_class = int(filters), int(units), int(embedding), int(self.n_class)
        rng = np.random.default_rng(seed)

        def glorot(shape, fan_in, fan_out):
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            return rng.uniform(-lim, lim, shape).astype(np.float32)
        K = glorot((kh, kw, 1, F), kh * kw, kh * kw * F)
        grus, d_in = [], api.conv2d_same_out_shape(T, D, strides)[1] * F
        for _ in range(int(n_gru)):
            W = glorot((d_in, 3 * H), d_in, 3 * H)
            _, _, vt = np.linalg.svd(rng.standard_normal((H, 3 * H)), full_matrices=False)
            grus.append((W, vt.astype(np.float32), np.zeros(3 * H, np.float32)))
            d_in = H
        Wd, Wh = glorot((H, E), H, E), glorot((E, n_class), E, n_class)
        import torch
        ctx = api.default_context()
        net = api.GruTrainer(ctx, (K, np.zeros(F, np.float32), strides), grus, (Wd, np.zeros(E, np.float32)), (Wh, np.zeros(n_class, np.float32)),
                             T=T, D=D, recurrent_activation=recurrent_activation, reset_after=False,
                             max_batch=max(1, min(1024, int(batch_size))))
        dev = "cuda:%d" % ctx.device
        xt, yt = torch.from_numpy(X_train).to(dev), torch.from_numpy(y_train).to(dev)   # the data stays on the device over the epochs
        xv, yv = torch.from_numpy(X_val).to(dev), torch.from_numpy(y_val).to(dev)
        hist = self._fit(net, xt, yt, xv, yv, rng, epochs, batch_size, lr, os.path.join(model_dir, "gru_training.log"))
        spk = ConvGruNet((net.read("conv_K"), net.read("conv_b"), strides),
                         [(net.read("gru%d_W" % i), net.read("gru%d_U" % i), net.read("gru%d_b" % i)) for i in range(int(n_gru))],
                         (net.read("dense_W"), net.read("dense_b")), recurrent_activation=recurrent_activation, reset_after=False,
                         input_shape=(T, D), device=ctx.device)
        save_model(spk, 'gru', model_dir)
        register_model('gru', spk)
        self.trainer_ = net
        return hist

    def test(self, X_train, Y_train, X_val, Y_val, model_name=_UNSET, spk_model=None):
        """d_vector.py:296-320, same positional signature: X = spkModel.predict(X) with the network ``model_name`` names (default
        'nn'; see _resolve_model), per-speaker centroids of X_train (one-hot Y_train), cosine distance of every X_val row to every
        centroid, accuracy of the arg-min.  The centroids stay available as ``self.centroids_`` (float64 (num, d) like the reference's
        ``avg``, d_vector.py:310)."""
        spk_model = _resolve_model(model_name, spk_model, 'nn')
        if spk_model is not None:
            X_train, X_val = spk_model.predict(X_train), spk_model.predict(X_val)
        num = Y_train.shape[1]
        lab = np.argmax(Y_train, axis=1)  # decoding the one-hot labels is index bookkeeping, not arithmetic
        avg = np.asarray(api.centroids(api.default_context(), np.asarray(X_train, dtype=np.float32), lab, num))
        self.centroids_ = avg.astype(np.float64)
        pred = identify(np.asarray(X_val, dtype=np.float32), avg)
        return (np.argmax(Y_val, axis=1) == pred).sum() / X_val.shape[0]

    def enroll(self, X_train, name, model_name=_UNSET, spk_model=None):
        """d_vector.py:322-344, same positional signature (default model 'lstm'): store the mean embedding under ``name`` (overwrites,
        like the reference)."""
        spk_model = _resolve_model(model_name, spk_model, 'lstm')
        if spk_model is not None:
            X_train = spk_model.predict(X_train)
        self._load()
        if name in self.d_vector:
            print("sample already exists")
        X = np.asarray(X_train, dtype=np.float32)
        self.d_vector[name] = np.asarray(api.centroids(api.default_context(), X, np.zeros(len(X), np.int32), 1))[0]
        self._save()

    def eval(self, target, model_name=_UNSET, spk_model=None):
        """d_vector.py:346-361, same positional signature (default model 'lstm'): the distances to every enrolled vector come from the
        GPU scorer; the decision is the reference's own scan in dict order — the running minimum starts at 1 and only a strictly
        smaller distance replaces it, so a NaN distance (zero-norm embedding or enrolment) is never selected and ties keep the first
        name.  Returns the name or None."""
        spk_model = _resolve_model(model_name, spk_model, 'lstm')
        if spk_model is not None:
            target = spk_model.predict(np.asarray(target, dtype=np.float32).reshape(1, -1))
        self._load()
        if not self.d_vector:
            return None
        names = list(self.d_vector.keys())
        C = np.stack([self.d_vector[n] for n in names]).astype(np.float32)
        r = api.cosine_identify(api.default_context(), np.asarray(target, dtype=np.float32).reshape(1, -1), C,
                                dist=True, argmin=False, minval=False)
        dist = np.asarray(r["dist"], dtype=np.float64).reshape(-1)
        min_distance, target_name = 1, None
        for name, dv in zip(names, dist):
            if min_distance > dv:
                min_distance, target_name = dv, name
        return target_name
