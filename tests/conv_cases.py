"""Seeded Conv2d geometries that are NOT unpadded square patch embeddings, shared by the CPU check of the oracle's im2col
(tests/test_oracle_golden.py) and the GPU tests of the conv search (tests/test_hip_conv_geometry.py).

Every case is valid for torch (output size >= 1 on both axes) and small enough that one ConvOracle evaluation takes seconds.
`assert_coverage` states what the list as a whole must contain; a CPU test runs it, so a change of the generator that loses a
property fails without a GPU."""
import numpy as np

METRICS = ["hessian", "L2_norm", "L1_norm", "cosine"]


def out_size(size, k, s, p, d):
    return (size + 2 * p - d * (k - 1) - 1) // s + 1


def conv_geometry_cases(n=16, seed=4242):
    rng = np.random.default_rng(seed)
    ics = [1, 3, 4, 5, 8]
    dils = [(1, 1), (2, 1), (1, 3), (1, 1), (1, 2), (3, 1), (2, 2), (1, 1)]
    cases = []
    for i in range(n):
        ic = ics[i % len(ics)]
        channelwise = i % 4 != 3
        metric = METRICS[(i + i // 4) % 4]
        kh, kw = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        sh, sw = int(rng.integers(1, 4)), int(rng.integers(1, 4))
        dh, dw = dils[i % len(dils)]
        ph, pw = int(rng.integers(0, 4)), int(rng.integers(0, 4))
        H, W = int(rng.integers(9, 27)), int(rng.integers(9, 27))
        b = 1 if i % 5 == 2 else int(rng.integers(2, 5))
        oc = int(rng.integers(3, 48))
        if i == 1:                       # a whole border of patches that see padding only (ph > dh * (kh - 1), likewise pw)
            kh, kw, ph, pw = 2, 3, 3, 5
        if i == 4:                       # K = 8 * 3 * 3 = 72: above 64 and not a multiple of 16; two column tiles, ragged
            kh, kw, oc = 3, 3, 200
        if i == 5:                       # K = 1 * 3 * 3 = 9 < 16
            kh, kw = 3, 3
        if i == 8:                       # K = 5 * 3 * 5 = 75, ragged oc over two tiles, one image
            kh, kw, oc = 3, 5, 131
        if i == 12:                      # ResNet-style 3x3 pad 1 and a 7x7 stride-2 pad-3 stem among the random ones
            kh, kw, sh, sw, ph, pw, dh, dw = 3, 3, 1, 1, 1, 1, 1, 1
        if i == 13:
            kh, kw, sh, sw, ph, pw, dh, dw = 7, 7, 2, 2, 3, 3, 1, 1
        while out_size(H, kh, sh, ph, dh) < 1:
            H += 3
        while out_size(W, kw, sw, pw, dw) < 1:
            W += 3
        # the activation search with packed conv planes: the channel-wise class on a difference metric (the layer-wise class
        # cannot search activations, conv.py:420; cosine is refused there, conv.py:505-506)
        a_bit = 8 if channelwise and metric != "cosine" and i % 2 == 0 else 32
        cases.append(dict(b=b, ic=ic, H=H, W=W, oc=oc, k=(kh, kw), stride=(sh, sw), padding=(ph, pw), dilation=(dh, dw),
                          channelwise=channelwise, metric=metric, w_bit=[8, 6, 4][(i + i // 3) % 3], a_bit=a_bit,
                          eq_n=[100, 37][i % 2], seed=500 + i))
    return cases


def case_id(c):
    p2 = lambda v: f"{v[0]}x{v[1]}"
    return (f"{'cw' if c['channelwise'] else 'lw'}-{c['metric'][:4]}-w{c['w_bit']}a{c['a_bit']}-b{c['b']}ic{c['ic']}-{c['H']}x{c['W']}-oc{c['oc']}"
            f"-k{p2(c['k'])}s{p2(c['stride'])}p{p2(c['padding'])}d{p2(c['dilation'])}-c{c['eq_n']}")


def dims(c):
    """(fh, fw, L, K, M) of a case."""
    fh = out_size(c["H"], c["k"][0], c["stride"][0], c["padding"][0], c["dilation"][0])
    fw = out_size(c["W"], c["k"][1], c["stride"][1], c["padding"][1], c["dilation"][1])
    return fh, fw, fh * fw, c["ic"] * c["k"][0] * c["k"][1], c["b"] * fh * fw


def make_tensors(c):
    """(weight, bias, x, out, grad) float32 numpy; out = F.conv2d(x, weight, bias, stride, padding, dilation)."""
    import torch
    rng = np.random.default_rng(c["seed"])
    oc, ic, (kh, kw) = c["oc"], c["ic"], c["k"]
    w = (rng.standard_normal((oc, ic, kh, kw)) * 0.05 * np.linspace(0.3, 3.0, oc)[:, None, None, None]).astype(np.float32)
    bias = (rng.standard_normal(oc) * 0.1).astype(np.float32)
    x = rng.standard_normal((c["b"], ic, c["H"], c["W"])).astype(np.float32)
    out = torch.nn.functional.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(bias), c["stride"], c["padding"],
                                     c["dilation"]).numpy()
    grad = (rng.standard_normal(out.shape) * 1e-3).astype(np.float32)
    return w, bias, x, out, grad


def assert_coverage(cases):
    D = [dims(c) for c in cases]
    has = lambda f: any(f(c, d) for c, d in zip(cases, D))
    assert has(lambda c, d: c["k"][0] != c["k"][1]), "kh != kw"
    assert has(lambda c, d: c["stride"][0] != c["stride"][1]), "sh != sw"
    assert has(lambda c, d: c["padding"][0] != c["padding"][1]), "ph != pw"
    assert has(lambda c, d: c["dilation"][0] > 1 and c["dilation"][1] == 1), "dilation on the h axis only"
    assert has(lambda c, d: c["dilation"][0] == 1 and c["dilation"][1] > 1), "dilation on the w axis only"
    assert has(lambda c, d: c["H"] != c["W"]), "H != W"
    assert has(lambda c, d: c["padding"][0] > c["dilation"][0] * (c["k"][0] - 1) or c["padding"][1] > c["dilation"][1] * (c["k"][1] - 1)), \
        "patches that are entirely padding"
    assert {c["ic"] for c in cases} >= {1, 3, 4, 5, 8}, "ic"
    assert has(lambda c, d: d[3] < 16), "K < 16"
    assert has(lambda c, d: d[3] > 64 and d[3] % 16), "K > 64, not a multiple of 16"
    assert has(lambda c, d: d[2] % 32), "L not a multiple of 32"
    assert has(lambda c, d: c["oc"] > 128 and c["oc"] % 32), "ragged oc over more than one column tile"
    assert has(lambda c, d: c["b"] == 1), "b = 1"
    assert {c["channelwise"] for c in cases} == {True, False}, "both classes"
    assert {c["metric"] for c in cases} == set(METRICS), "metrics"
    for cw in (True, False):
        assert {c["metric"] for c in cases if c["channelwise"] == cw} >= {"hessian", "cosine"}, "hessian and cosine on both classes"
    assert {c["w_bit"] for c in cases} == {8, 6, 4}, "w_bit"
    assert sum(c["a_bit"] == 8 for c in cases) >= 3, "a_bit = 8 cases"
    assert all(c["channelwise"] and c["metric"] != "cosine" for c in cases if c["a_bit"] == 8)
    assert all(d[0] >= 1 and d[1] >= 1 for d in D)
