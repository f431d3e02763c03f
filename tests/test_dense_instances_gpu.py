"""Every kernel behind ssp_dense_forward and ssp_dnn_forward (csrc/cosine.hip cosine_reg_kernel<NQ = 8, 16, 24, 32; DENSE>, csrc/dense.hip
dense_kernel, csrc/dnn_chain.hip dnn_chain_kernel + dnn_pack_kernel) against float64 at its edges: widths on both sides of every
instance's range, unit counts and batch sizes around the tiles, odd and even k-slab counts, chains of depth 1 to 8 and the split in
front of depth 9, linear hidden layers, and input that is not finite.

The yardstick is tests/dense_cases.py: the oracle, the derived band and the three input kinds; tests/test_dense_instances_host.py checks
the yardstick itself.  The rules: gaussian — inside the band elementwise; exact — the bits of float32(ref64); probe — the weights' own
bits; batch invariance and host against device — bit identity; non-finite — NaN, +inf and -inf where the oracle has them, everything
else inside the band, every other sample untouched.  Every call prints what it measured as a `dense_accuracy {json}` line (pytest -s);
profiles/dense_accuracy.md is made of those lines."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_cases as K              # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from speech_signal_processing_amd import api
    return api


def record(tag="dense_accuracy", **kw):
    print(tag + " " + json.dumps({k: (float("%.4g" % v) if isinstance(v, float) else v) for k, v in kw.items()}))


def layer_forward(api, c, X=None):
    (W, b, act), = c["layers"]
    return api.dense_forward(api.default_context(), c["X"] if X is None else X, np.ascontiguousarray(W.T), b, relu=act == "relu")


def make_net(api, layers):
    return api.DnnForward(api.default_context(), [(np.ascontiguousarray(W.T), b, act == "relu") for W, b, act in layers])


def net_forward(api, c, X=None):
    net = make_net(api, c["layers"])
    try:
        return np.asarray(net.forward(c["X"] if X is None else X))
    finally:
        net.close()


def check(got, c, instance, want=None):
    """the one comparison of a finite case; -> max error / band"""
    what = (instance, c["kind"], c["dims"], c["N"], [a for _, _, a in c["layers"]], [b is not None for _, b, _ in c["layers"]])
    ref, band = K.band_of(c["X"], c["layers"])
    assert got.shape == ref.shape and got.dtype == np.float32, what
    ratio = K.ratio_of(got, ref, band)
    record(instance=instance, case=c["kind"], shape=c["dims"] if len(c["dims"]) < 6 else [c["dims"][0], "%d x %d" % (len(c["dims"]) - 1, c["dims"][1])],
           N=c["N"], bias=c["layers"][0][1] is not None, relu=[a == "relu" for _, _, a in c["layers"]], max_err_over_band=ratio)
    assert np.isfinite(got).all(), what
    if c["kind"] == "exact":
        w32 = ref.astype(np.float32)
        assert np.array_equal(got, w32), (what, "exact inputs", np.argwhere(got != w32)[:4])
    elif c["kind"] == "probe":
        assert got.tobytes() == want.tobytes(), (what, "the weights' bits", np.argwhere(got != want)[:4])
    else:
        assert ratio <= 1.0, (what, "band", ratio, np.argwhere(np.abs(got - ref) > band)[:4])
    return ratio


def sweep_layers(api, shapes, instance_of):
    for i, (d, u, n) in enumerate(shapes):
        for j, kind in enumerate(("gaussian", "exact")):
            bias, relu = K.COMBOS[(i + j) % 4]
            c = K.layer_case(kind, d, u, n, bias, relu)
            check(layer_forward(api, c), c, instance_of(d))
    for i, (d, u) in enumerate(sorted(set((d, u) for d, u, _ in shapes))):
        bias, relu = K.COMBOS[(i + 1) % 4]
        c, want = K.probe(d, u, bias=bias, relu=relu)
        check(layer_forward(api, c), c, instance_of(d), want)
        if i % 7 == 0:      # the plain probe: no bias, linear
            c, want = K.probe(d, u)
            check(layer_forward(api, c), c, instance_of(d), want)


# ------------------------------------------------------------------------------------------------- the register GEMM
@pytest.mark.parametrize("nq", sorted(K.REG_D))
def test_register_gemm(api, nq):
    """cosine_reg_kernel<NQ, true>: every d_in of the instance (both ends of its range among them) with every units at N = 33 and 129 and
    every N at units = 36 and 257; gaussian and exact at every shape, the probe at every (d_in, units); bias and ReLU rotate"""
    sweep_layers(api, K.reg_shapes(nq), lambda d: K.instance_name(K.kernel_of(d)))


# ------------------------------------------------------------------------------------------------- the tiled GEMM
def test_tiled_gemm(api):
    """dense_kernel: odd and even slab counts, every d_in % 4, units off the multiple of 4 above 128, N across the 128-sample workgroup"""
    sweep_layers(api, K.tiled_shapes(), lambda d: "dense_kernel n_kc=%d" % K.n_kc(d))


def test_tiled_gemm_below_257_against_the_register_gemm(api, monkeypatch):
    """SSP_DENSE_NO_REG (read per call) sends d_in <= 256 to dense_kernel: 1, 2, 3, 4 and 8 slabs, where the look-ahead loads are all out
    of range.  The register GEMM answers the same inputs; both sit inside the band of one oracle (they need not agree bit for bit)."""
    cases = []
    for i, (d, u, n) in enumerate(K.noreg_shapes()):
        for j, kind in enumerate(("gaussian", "exact")):
            bias, relu = K.COMBOS[(i + j) % 4]
            cases.append(K.layer_case(kind, d, u, n, bias, relu))
        cases.append(K.probe(d, u, bias=i % 2 == 1))
    monkeypatch.delenv("SSP_DENSE_NO_REG", raising=False)
    for c in cases:
        c, want = c if isinstance(c, tuple) else (c, None)
        check(layer_forward(api, c), c, K.instance_name(K.kernel_of(c["dims"][0])), want)
    monkeypatch.setenv("SSP_DENSE_NO_REG", "1")
    for c in cases:
        c, want = c if isinstance(c, tuple) else (c, None)
        check(layer_forward(api, c), c, "dense_kernel n_kc=%d (register GEMM off)" % K.n_kc(c["dims"][0]), want)


# ------------------------------------------------------------------------------------------------- the chain
def _net_id(d):
    return "x".join(map(str, d)) if len(d) < 6 else "%dx%dx..(%d)" % (d[0], d[1], len(d) - 1)


@pytest.mark.parametrize("dims", K.NETS, ids=_net_id)
def test_packed_network(api, dims):
    """ssp_dnn: N over 1, 15, 16, 17, 63, 64, 65, 129, gaussian and exact, the ReLU patterns rotating, every bias None once per kind"""
    name = " > ".join(K.instance_name(k) for k in K.route(list(dims)))
    for kind, n, bias, relu in K.net_cases(dims):
        c = K.make(kind, list(dims), n, bias, relu)
        check(net_forward(api, c), c, name)


@pytest.mark.parametrize("d,u", K.CHAIN_PROBES)
def test_chain_probe(api, d, u):
    """a chain of one layer on the identity: every position of dnn_pack_kernel's image is read once"""
    for bias in (False, True):
        c, want = K.probe(d, u, bias=bias)
        assert K.route(c["dims"]) == [("chain", 1)]
        check(net_forward(api, c), c, "dnn_chain depth 1", want)


# ------------------------------------------------------------------------------------------------- properties
PROPERTY_CASES = (("layer", [130, 36]), ("layer", [289, 130]), ("layer", [64, 257]), ("net", [40, 32, 16]), ("net", [5, 17, 15, 16, 3]),
                  ("net", [10, 300, 20, 8]), ("net", [1274, 256, 256, 256, 256]))


@pytest.mark.parametrize("how,dims", PROPERTY_CASES, ids=lambda v: v if isinstance(v, str) else _net_id(v))
def test_batch_invariance_host_device_and_empty_batch(api, how, dims):
    """a sample's output bits do not depend on its batch (a permutation, the first 1, 17 and 65 rows); a torch-tensor call gives the
    host-array call's bits; N = 0 returns an empty (0, units) array"""
    import torch
    c = K.gaussian(dims, 129, relu="all" if how == "layer" else "ref")
    X = c["X"]
    if how == "layer":
        (W, b, act), = c["layers"]
        Wt = np.ascontiguousarray(W.T)
        ctx = api.default_context()
        fwd = lambda x: api.dense_forward(ctx, x, Wt, b, relu=True)                                        # noqa: E731
        dev = lambda x: api.dense_forward(ctx, torch.from_numpy(x).cuda(), torch.from_numpy(Wt).cuda(),    # noqa: E731
                                          torch.from_numpy(b).cuda(), relu=True).cpu().numpy()
    else:
        net = make_net(api, c["layers"])
        fwd = lambda x: np.asarray(net.forward(x))                                                         # noqa: E731
        dev = lambda x: net.forward(torch.from_numpy(x).cuda()).cpu().numpy()                              # noqa: E731
    full = fwd(X)
    check(full, c, how + " batch")
    perm = np.random.default_rng(5).permutation(len(X))
    assert fwd(np.ascontiguousarray(X[perm])).tobytes() == full[perm].tobytes(), "a permutation of the batch moves bits"
    for n in (1, 17, 65):
        assert fwd(np.ascontiguousarray(X[:n])).tobytes() == full[:n].tobytes(), "the first %d rows alone differ" % n
    assert dev(X).tobytes() == full.tobytes(), "device call differs from host call"
    empty = fwd(np.zeros((0, dims[0]), np.float32))
    assert empty.shape == (0, dims[-1]) and empty.dtype == np.float32
    empty_dev = dev(np.zeros((0, dims[0]), np.float32))
    assert empty_dev.shape == (0, dims[-1])


# ------------------------------------------------------------------------------------------------- the non-finite table
def run_table(api, dims, relu, forward, instance):
    clean_c, table = K.nonfinite_table(list(dims), K.NONFINITE_N, relu=relu)
    clean = forward(clean_c["layers"], clean_c["X"])
    check(clean, clean_c, instance)
    failed = []
    for e in table:
        ref, band = K.band_of(e["X"], e["layers"])
        got = forward(e["layers"], e["X"])
        kind_ok = K.same_kind(got, ref)
        ratio = K.ratio_of(got, ref, band)
        others_ok = True
        if e["sample"] is not None:
            others = np.arange(K.NONFINITE_N) != e["sample"]
            others_ok = got[others].tobytes() == clean[others].tobytes()
        ok = bool(kind_ok and ratio <= 1.0 and others_ok)
        record("dense_nonfinite", instance=instance, shape=list(dims), relu=relu, case=e["name"], value=e["value"], kind_matches=bool(kind_ok),
               max_err_over_band=ratio, other_rows_untouched=bool(others_ok), passed=ok)
        if not ok:
            failed.append((e["name"], "kind" if not kind_ok else "band %.3g" % ratio if ratio > 1.0 else "other rows"))
    assert not failed, (instance, list(dims), relu, "%d of %d rows of the table fail" % (len(failed), len(table)), failed)


@pytest.mark.parametrize("relu", ("all", "none"), ids=("relu", "linear"))
@pytest.mark.parametrize("d,u", K.NONFINITE_LAYERS)
def test_nonfinite_layer(api, d, u, relu):
    """NaN, +inf, -inf in one sample (column 0, column d_in - 1, the last partial group of four), NaN in one weight and one bias entry:
    Y is NaN / +inf / -inf exactly where the float64 oracle is, finite elements stay inside the band, every other sample keeps its bits.
    (ReLU by fmaxf returned 0 for a NaN: every NaN row of the ReLU cases failed before the select.)"""
    ctx = api.default_context()

    def forward(layers, X):
        (W, b, act), = layers
        return api.dense_forward(ctx, X, np.ascontiguousarray(W.T), b, relu=act == "relu")
    run_table(api, [d, u], relu, forward, K.instance_name(K.kernel_of(d)))


@pytest.mark.parametrize("dims,relu", K.NONFINITE_NETS, ids=lambda v: v if isinstance(v, str) else _net_id(v))
def test_nonfinite_net(api, dims, relu):
    """the same table through ssp_dnn.  [5, 17, 15, 16, 3] is all linear: its padded hidden units hold 0 * inf = NaN, which reached every
    real unit of the next layer as 0 * NaN before the padded units were zeroed; the oracle carries +-inf to the output."""
    def forward(layers, X):
        net = make_net(api, layers)
        try:
            return np.asarray(net.forward(X))
        finally:
            net.close()
    run_table(api, dims, relu, forward, " > ".join(K.instance_name(k) for k in K.route(list(dims))))
