"""No GPU: the host side of the one-kernel window attention core (P4V_WATTN_ONE_KERNEL, bit 4 of p4v_wattn_desc.pv.reserved) --
the sizing answers for the descriptor as given, the descriptor did not grow, the version and the header say so."""
import ctypes as C
import os
import re

import pytest

from tests.test_fused_window_attention_host import _desc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from ptq4vit_amd import _lib
    return _lib.load()


def _sizes(lib, **kw):
    from ptq4vit_amd import _lib
    two, one = _desc(**kw), _desc(**kw)
    one.pv.reserved |= _lib.WATTN_ONE_KERNEL
    return lib.p4v_wattn_workspace_bytes(C.byref(two)), lib.p4v_wattn_workspace_bytes(C.byref(one))


@pytest.mark.parametrize("kw, served", [(dict(N=49), True), (dict(windows=4, heads=4, N=144), True), (dict(N=49, D=12, bits=6, sos=False), True),
                                        (dict(N=161), False), (dict(N=49, D=64), False)], ids=["n49", "n144", "d12_plain", "n161", "dv64"])
def test_sizing_answers_for_the_descriptor_as_given(lib, kw, served):
    two, one = _sizes(lib, **kw)
    assert two > 0 and (0 < one < two if served else one == two), (kw, one, two)


def test_descriptor_version_and_header(lib):
    from ptq4vit_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ptq4vit_hip.h")).read()
    assert int(re.search(r"#define\s+P4V_WATTN_ONE_KERNEL\s+(\d+)", hdr).group(1)) == _lib.WATTN_ONE_KERNEL == 16
    assert C.sizeof(_lib.WattnDesc) == 2 * C.sizeof(_lib.MatMulDesc) + 8          # qk, pv, n_windows, has_mask: no new field
    assert lib.p4v_version() >= 147
    assert _lib.LAUNCH_KINDS[20] == "k_wattn_qkpv"
