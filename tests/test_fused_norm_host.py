"""No GPU: the host side of the fused LayerNorm producer -- the descriptor and tensor records against _lib's mirrors, the version,
the sizing run's arithmetic, and the envelope's refusals (nothing is launched: every pointer is a fake that is never dereferenced)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ptq4vit_amd import _lib
    return _lib.load()


def _lin(M, K, N, **kw):
    from ptq4vit_amd import _lib
    d = _lib.LinearDesc(1, M, K, N, 1, 1, 1, 8, 8, _lib.METRICS["L2_norm"], 1, 1, 0, 0, 1, _lib.RESERVED_FORWARD_ONLY)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _ln(rows, Cc, window=None):
    from ptq4vit_amd import _lib
    return _lib.LnDesc(rows, Cc, 1e-6, *((1,) + window if window else (0, 0, 0, 0, 0)), 0)


def _members(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    return tuple(re.findall(r"\*?\s*([A-Za-z_][A-Za-z0-9_]*)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S)))


def test_records_version_and_exports(lib):
    from ptq4vit_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ptq4vit_hip.h")).read()
    assert _members(hdr, "p4v_ln_desc") == tuple(n for n, _ in _lib.LnDesc._fields_) and C.sizeof(_lib.LnDesc) == 40
    assert _members(hdr, "p4v_ln_linear_tensors") == _lib.LnLinearTensors.POINTERS + ("ws_bytes",)
    assert _members(hdr, "p4v_ln_mlp_tensors") == _lib.LnMlpTensors.POINTERS + ("ws_bytes",)
    assert C.sizeof(_lib.LinearDesc) == 64 and C.sizeof(_lib.MlpDesc) == 128              # no existing descriptor changed size
    assert lib.p4v_version() >= 148 and _lib.LAUNCH_KINDS[21] == "k_ln_pack"
    assert {"p4v_ln_linear_workspace_bytes", "p4v_ln_linear_quant_forward", "p4v_ln_mlp_workspace_bytes", "p4v_ln_mlp_quant_forward",
            "p4v_debug_ln_planes"} <= set(_lib.EXPORTS)
    info = (C.c_uint64 * 5)()
    assert lib.p4v_debug_ln_planes(info) == -1 and b"no p4v_ln_linear_quant_forward" in lib.p4v_last_error()


@pytest.mark.parametrize("M,K,N", [(5, 96, 64), (394, 192, 768)])
def test_sizing_is_the_linear_call_with_the_plane_carved_first(lib, M, K, N):
    """ln_linear: the Linear's forward with its row plane [Mp][roundup64(K)] carved in front instead of inside the pass -- the
    same bytes up to the arena's 256-byte rounding.  ln_mlp: the MLP chain's need plus at most fc1's row plane, which now outlives
    the producer."""
    from ptq4vit_amd import _lib
    up = lambda v, m: (v + m - 1) // m * m
    lin, ln = _lin(M, K, N), _ln(M, K)
    need, plain = lib.p4v_ln_linear_workspace_bytes(C.byref(ln), C.byref(lin)), lib.p4v_linear_workspace_bytes(C.byref(lin))
    plane = up(M, 128) * up(K, 64)
    assert need >= plane and abs(need - plain) <= 1024, (need, plain)
    mlp = _lib.MlpDesc(_lin(M, K, N), _lin(M, N, K))
    need2, plain2 = lib.p4v_ln_mlp_workspace_bytes(C.byref(ln), C.byref(mlp)), lib.p4v_mlp_workspace_bytes(C.byref(mlp))
    assert plain2 <= need2 <= plain2 + plane + 1024, (need2, plain2)
    assert lib.p4v_ln_linear_workspace_bytes(None, C.byref(lin)) == 0 and lib.p4v_ln_mlp_workspace_bytes(C.byref(ln), None) == 0


def test_envelope_refusals_launch_nothing(lib):
    from ptq4vit_amd import _lib, engine
    before = engine.launch_counters()

    def refused(ln, lin, code, msg, **ptrs):
        t = _lib.LnLinearTensors(**{n: 64 for n in _lib.LnLinearTensors.POINTERS})
        t.ws_bytes = 1 << 30
        for k, v in ptrs.items():
            setattr(t, k, v)
        if not ptrs:
            assert lib.p4v_ln_linear_workspace_bytes(C.byref(ln), C.byref(lin)) == 0 and msg in lib.p4v_last_error(), lib.p4v_last_error()
        assert lib.p4v_ln_linear_quant_forward(C.byref(ln), C.byref(lin), C.byref(t), None) == code and msg in lib.p4v_last_error(), lib.p4v_last_error()

    refused(_ln(8, 2052), _lin(8, 2052, 64), -2, b"multiple of 4 up to 2048")
    refused(_ln(8, 98), _lin(8, 98, 64), -2, b"multiple of 4 up to 2048")
    refused(_ln(8, 96), _lin(9, 96, 64), -1, b"are not the Linear's input")
    refused(_ln(8, 96), _lin(8, 128, 64), -1, b"are not the Linear's input")
    refused(_ln(128, 96, (8, 8, 4, 4)), _lin(128, 96, 64), -1, b"window map")          # shift = ws
    refused(_ln(128, 96, (8, 16, 3, 0)), _lin(128, 96, 64), -1, b"window map")         # H % ws != 0
    refused(_ln(100, 96, (8, 8, 4, 0)), _lin(100, 96, 64), -1, b"window map")          # rows % (H W) != 0
    refused(_ln(8, 96), _lin(8, 96, 64, n_a=2), -2, b"n_H = n_a = 1")
    refused(_ln(8, 96), _lin(8, 96, 64, twin_postgelu=1), -2, b"twin_postgelu")
    refused(_ln(8, 96), _lin(8, 96, 64, reserved=5), -2, b"int8 planes only")
    refused(_ln(8, 96), _lin(8, 96, 64), -1, b"null pointer", gamma=0)
    refused(_ln(8, 96), _lin(8, 96, 64), -1, b"aligned to 16 bytes", x=72)
    refused(_ln(8, 96), _lin(8, 96, 64), -3, b"workspace too small", ws_bytes=1)
    assert engine.launch_counters() == before
