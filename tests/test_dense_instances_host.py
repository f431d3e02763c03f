"""The yardstick of tests/test_dense_instances_gpu.py checked by itself (numpy, no GPU): the derived band holds a float32 restatement of
every gaussian case in two accumulation orders, and is not slack — a dropped last input column, a dropped last bias, a skipped k-slab
and a ReLU on the last layer each leave it (or break the exact cases' equality); the exact cases are proved order-independent in int64;
the probe expects the weights' own bits; kernel_of / chain_from sit on the right side of every edge; the oracle keeps a NaN under ReLU."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_cases as K  # noqa: E402

ORDERS = ("strict", "pairwise")


def _layer_shapes():
    out = []
    for nq in K.REG_D:
        out += K.reg_shapes(nq)
    return out + K.tiled_shapes() + K.noreg_shapes()


def _host_subset(shapes):
    """the float32 restatement costs N x d_in x units per case: every d_in and every units of the tables once at the largest N that the
    table pairs it with, which is where the restatement's error is largest"""
    best = {}
    for d, u, n in shapes:
        for key in (("d", d), ("u", u)):
            if key not in best or n * u * d > best[key][2] * best[key][1] * best[key][0]:
                best[key] = (d, u, n)
    return sorted(set(best.values()))


def test_band_holds_float32_restatement_of_every_gaussian_layer():
    worst = {}
    for i, (d, u, n) in enumerate(_layer_shapes()):
        bias, relu = K.COMBOS[i % 4]
        c = K.layer_case("gaussian", d, u, n, bias, relu)
        ref, band = K.band_of(c["X"], c["layers"])
        for order in ORDERS:
            r = K.ratio_of(K.emu32(c["X"], c["layers"], order), ref, band)
            assert r <= 1.0, (d, u, n, order, r)
            fam = K.kernel_of(d)[0]
            worst[(fam, order)] = max(worst.get((fam, order), 0.0), r)
    print("dense_host_ratio " + json.dumps({"%s %s" % k: float("%.4g" % v) for k, v in sorted(worst.items())}))
    assert all(v > 0 for v in worst.values())


@pytest.mark.parametrize("dims", K.NETS, ids=lambda d: "x".join(map(str, d)) if len(d) < 6 else "%dx%dx..(%d)" % (d[0], d[1], len(d) - 1))
def test_band_holds_float32_restatement_of_every_net(dims):
    worst = 0.0
    for i, pattern in enumerate(K.NET_RELU):
        c = K.gaussian(dims, 65, bias=i != 1, relu=K.net_relu(dims, i))
        ref, band = K.band_of(c["X"], c["layers"])
        for order in ORDERS:
            r = K.ratio_of(K.emu32(c["X"], c["layers"], order), ref, band)
            assert r <= 1.0, (dims, pattern, order, r)
            worst = max(worst, r)
    print("dense_host_ratio " + json.dumps({"net": list(dims), "max_err_over_band": float("%.4g" % worst)}))
    assert worst > 0


def _exact_cases():
    for i, (d, u, n) in enumerate(_host_subset(_layer_shapes())):
        bias, relu = K.COMBOS[(i + 1) % 4]
        yield K.layer_case("exact", d, u, n, bias, relu)
    for dims in K.NETS:
        for kind, n, bias, relu in K.net_cases(dims):
            if kind == "exact":
                yield K.exact(dims, n, bias=bias, relu=relu)


def test_exact_cases_are_order_independent_and_reach_the_edges():
    n_cases = 0
    for c in _exact_cases():
        assert K.exact_bound(c) < 2 ** 24, (c["dims"], c["N"], K.exact_bound(c))
        assert c["X"][-1, -1] != 0
        for l, (W, b, _) in enumerate(c["layers"]):
            assert np.any(W[-1] != 0) and np.any(W[:, 0] != 0) and np.any(W[:, -1] != 0), (c["dims"], l)
            if l > 0:
                assert (np.count_nonzero(W, axis=0) <= 2).all() and np.abs(W).max() == 1
        n_cases += 1
    assert n_cases > 60
    # both orders of the restatement give float32(ref64) bit for bit
    for c in (K.layer_case("exact", 1274, 260, 40, True, False), K.exact([40] + [24] * 9, 65), K.exact([1274, 256, 256, 256, 256], 17),
              K.exact([10, 300, 20, 8], 33, relu="none")):
        want = K.ref64(c["X"], c["layers"]).astype(np.float32)
        assert np.array_equal(want.astype(np.float64), K.ref64(c["X"], c["layers"]))
        for order in ORDERS:
            assert np.array_equal(K.emu32(c["X"], c["layers"], order), want), (c["dims"], order)
        assert np.count_nonzero(want) > want.size // 8


def test_probe_expects_the_weights_own_bits():
    for d, u in ((5, 3), (64, 33), (200, 256), (256, 7), (289, 130)):
        c, want = K.probe(d, u)
        W = c["layers"][0][0]
        assert want.tobytes() == W.tobytes() and np.array_equal(c["X"], np.eye(d, dtype=np.float32))
        assert (np.abs(W) >= np.finfo(np.float32).tiny).all()
        for order in ORDERS:
            assert K.emu32(c["X"], c["layers"], order).tobytes() == want.tobytes()
        cb, wb = K.probe(d, u, bias=True, relu=True)
        Wb, bb, _ = cb["layers"][0]
        assert wb.dtype == np.float32 and np.array_equal(wb, np.maximum(Wb + bb[None, :], np.float32(0)))
        assert K.emu32(cb["X"], cb["layers"], "strict").tobytes() == wb.tobytes()
        ref, band = K.band_of(cb["X"], cb["layers"])
        assert K.ratio_of(wb, ref, band) <= 1.0


def test_kernel_choice_on_both_sides_of_every_edge():
    assert [K.kernel_of(d) for d in (1, 64, 65, 128, 129, 192, 193, 256, 257, 1274)] == [
        ("reg", 8), ("reg", 8), ("reg", 16), ("reg", 16), ("reg", 24), ("reg", 24), ("reg", 32), ("reg", 32), ("tiled",), ("tiled",)]
    assert [K.n_kc(d) for d in K.NOREG_D] == [1, 1, 1, 2, 2, 3, 3, 4, 8]
    assert sorted(set(K.n_kc(d) % 2 for d in K.TILED_D)) == [0, 1] and sorted(set(d % 4 for d in K.TILED_D)) == [0, 1, 2, 3]
    want = {(1, 1): 0, (3, 1, 7): 0, (5, 17, 15, 16, 3): 0, (255, 256, 255, 4): 0, (256, 200, 256, 252): 0, tuple([40] + [24] * 8): 0,
            tuple([40] + [24] * 9): 1, (10, 300, 20, 8): 2, (256, 257, 256): 2, (1274, 256, 256, 256, 256): 1}
    assert set(want) == set(tuple(d) for d in K.NETS)
    for dims, frm in want.items():
        assert K.chain_from(list(dims)) == frm, (dims, K.chain_from(list(dims)))
    assert K.route([40] + [24] * 9) == [("reg", 8), ("chain", 8)]
    assert K.route([10, 300, 20, 8]) == [("reg", 8), ("tiled",), ("chain", 1)]
    assert K.route([256, 257, 256]) == [("reg", 32), ("tiled",)]
    assert K.route([1274, 256, 256, 256, 256]) == [("tiled",), ("chain", 3)]
    assert K.chain_from([257, 256]) == 1 and K.chain_from([256, 256]) == 0 and K.chain_from([256, 257]) == 1


MUTATION_CASES = {
    "drop_last_column": [("gaussian", [64, 33], 33, True, "none"), ("gaussian", [289, 130], 129, True, "none"), ("exact", [64, 33], 33, True, "none"),
                         ("gaussian", [40] + [24] * 8, 17, True, "ref"), ("exact", [1274, 260], 40, False, "none")],
    "drop_last_bias": [("gaussian", [64, 33], 33, True, "none"), ("gaussian", [1274, 260], 40, True, "all"), ("gaussian", [256, 200, 256, 252], 17, True, "ref"),
                       ("exact", [1274, 256, 256, 256, 256], 17, True, "ref")],
    "skip_slab": [("gaussian", [64, 33], 33, True, "none"), ("gaussian", [1274, 260], 40, True, "none"), ("exact", [289, 130], 129, True, "none"),
                  ("exact", [1274, 256, 256, 256, 256], 17, True, "ref")],
    "relu_on_last": [("gaussian", [64, 33], 33, True, "none"), ("exact", [289, 130], 129, True, "none"), ("gaussian", [5, 17, 15, 16, 3], 17, True, "none"),
                     ("exact", [1274, 256, 256, 256, 256], 17, True, "ref")],
}


@pytest.mark.parametrize("mutation", K.MUTATIONS)
def test_band_is_not_slack(mutation):
    """each mutation of the restatement leaves the band (gaussian) or breaks bit equality (exact) on every case meant to catch it, while
    the restatement itself passes.  (The band of a stack compounds |W|' E per layer and is wide at the end of the four-layer network:
    there the exact kind is the one that catches a mutation.)"""
    for kind, dims, n, bias, relu in MUTATION_CASES[mutation]:
        c = K.make(kind, dims, n, bias, relu)
        ref, band = K.band_of(c["X"], c["layers"])
        good, bad = K.emu32(c["X"], c["layers"]), K.emu32(c["X"], c["layers"], mutate=mutation)
        if kind == "exact":
            assert np.array_equal(good, ref.astype(np.float32))
            assert not np.array_equal(bad, ref.astype(np.float32)), (mutation, dims)
        else:
            assert K.ratio_of(good, ref, band) <= 1.0
            r = K.ratio_of(bad, ref, band)
            print("dense_host_mutation " + json.dumps({"mutation": mutation, "dims": dims if len(dims) < 6 else dims[:2] + ["..."], "ratio": float("%.4g" % r)}))
            assert r > 1.0, (mutation, dims, r)


def test_oracle_keeps_nan_under_relu_and_the_table_is_what_it_says():
    from oracle import ref_cpu as O
    y = O.dense_net_forward(np.array([[np.nan, 1.0], [1.0, 1.0]]), [(np.ones((2, 2)), None, "relu")])
    assert np.isnan(y[0]).all() and np.array_equal(y[1], [2.0, 2.0])
    assert np.isnan(np.maximum(np.nan, 0.0))
    for dims, relu in [(list(s), "all") for s in K.NONFINITE_LAYERS] + [(list(d), r) for d, r in K.NONFINITE_NETS]:
        c, table = K.nonfinite_table(dims, K.NONFINITE_N, relu=relu)
        assert all((W != 0).all() and np.array_equal(W, np.rint(W)) for W, _, _ in c["layers"])
        clean, band = K.band_of(c["X"], c["layers"])
        assert np.isfinite(clean).all() and (band > 0).all()
        kinds = set()
        for e in table:
            ref, band = K.band_of(e["X"], e["layers"])
            assert np.isfinite(band).all()
            if e["sample"] is not None:
                others = np.arange(K.NONFINITE_N) != e["sample"]
                assert np.array_equal(ref[others], clean[others]) and not np.isfinite(ref[e["sample"]]).all()
                row = ref[e["sample"]]
                kinds |= {("nan", bool(np.isnan(row).any())), ("inf", bool(np.isinf(row).any()))}
                if e["value"] != "nan":      # the sign structure of the weights carries +-inf, not inf - inf, to the output
                    assert not np.isnan(row).any(), (dims, e["name"])
                    assert np.isinf(row).any() or relu != "none"
                # the restatement obeys the rule the kernels are held to
                emu = K.emu32(e["X"], e["layers"])
                assert K.same_kind(emu, ref) and K.ratio_of(emu, ref, band) <= 1.0, (dims, e["name"])
            else:
                assert np.isnan(ref).any()
        assert ("nan", True) in kinds and ("inf", True) in kinds, (dims, kinds)


def test_fuzz_tool_restates_the_band():
    """tools/fuzz_scoring.py carries the one-layer band as a line of its own (it imports nothing from tests/): the same numbers as
    K.band_of, and its dense layers are no longer all linear"""
    import re
    src = open(os.path.join(K.ROOT, "tools", "fuzz_scoring.py")).read()
    m = re.search(r"^dense_band = (lambda X, W, b: .*)$", src, re.M)
    assert m and "and False" not in src
    f = eval(m.group(1), {"np": np})
    for d, u, n in ((1, 3, 5), (33, 129, 127), (1274, 256, 7)):
        c = K.gaussian([d, u], n, relu="all")
        W, b, _ = c["layers"][0]
        assert np.array_equal(f(c["X"], W, b), K.band_of(c["X"], c["layers"])[1])


def test_selection_rules_restate_the_host_code():
    """the lines kernel_of, chain_from and n_kc mirror, read from the sources as they stand"""
    csrc = os.path.join(K.ROOT, "speech_signal_processing_amd", "csrc")
    dense, cosine, chain = (open(os.path.join(csrc, f)).read() for f in ("dense.hip", "cosine.hip", "dnn_chain.hip"))
    assert 'if (d_in <= 256 && !getenv("SSP_DENSE_NO_REG"))' in dense
    assert "constexpr int DBK = %d;" % K.DBK in dense and "const int n_kc = (d + DBK - 1) / DBK;" in dense
    assert "const int nq = d_in <= 64 ? 8 : (d_in <= 128 ? 16 : (d_in <= 192 ? 24 : 32));" in cosine
    assert "constexpr int CH_W = %d;" % K.CH_W in chain and "constexpr int CH_MAXL = %d;" % K.CH_MAXL in chain
    assert "while (from > 0 && dims[from - 1] <= CH_W && dims[from] <= CH_W && n_layers - (from - 1) <= CH_MAXL) --from;" in chain
