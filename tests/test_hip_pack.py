"""GPU, bit-exact: the candidate planes of the search (k_pack, and k_pack1 for a single plane) through p4v_debug_pack_cands.

Every plane is compared byte for byte with numpy's IEEE clamp(rint(x / s), lo, hi): the four layouts, the 8- and 6-bit grids,
values on and around every grid breakpoint, zeros, saturation, NaN / +-inf and a scale whose reciprocal overflows, ragged rows
with a partial last 16-element run (padding bytes are zero).  Pruned launches -- a device-side candidate range, optional
`done` flags, and what the host knows of the range (nothing, its length) -- pack exactly the candidates of the range that
are not flagged and leave every other byte of the destination as it was; the launch that knows the length of the range and
the one that knows nothing write the same buffer.  The single-plane kernel equals k_pack with one candidate.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ptq4vit_amd import engine
    return engine


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _grid(v, lo, hi):
    """fminf(fmaxf(rintf(v), lo), hi) with C's NaN rules (fmaxf / fminf return the other operand)."""
    return np.fmin(np.fmax(np.rint(v), np.float32(lo)), np.float32(hi))


def _around(points):
    p = np.asarray(points, np.float32)
    return np.concatenate([p, np.nextafter(p, np.float32(np.inf)), np.nextafter(p, np.float32(-np.inf))])


def _i8(v):
    return (v.astype(np.int64) & 0xFF).astype(np.uint8).view(np.int8)


SPECIALS = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 3.0e38, -3.0e38, 1e-30, -1e-30], np.float32)


def _scales(C, base, overflow=False):
    """C candidate scales on the search's grid of multipliers (0.01 .. 1.2 of `base`)."""
    s = (np.float32(base) * np.linspace(0.01, 1.2, C, dtype=np.float32)).astype(np.float32)
    if overflow:
        s[C // 2] = np.float32(2.0e-39)             # 1 / s overflows: the division path
    return s


def _source(rows, cols, scales, bit, seed):
    """[rows][cols]: every breakpoint (k + 0.5) s and grid point k s of a few of the scales with both float neighbours, the
    specials, random values for the rest -- shuffled, so that specials also land in the last, partial run of a row."""
    q = 2 ** (bit - 1)
    rng = np.random.default_rng(seed)
    k = np.arange(-q - 2, q + 2, dtype=np.float32)
    pick = scales[np.unique(np.linspace(0, len(scales) - 1, 4).astype(int))]
    vals = np.concatenate([_around((k + 0.5) * s) for s in pick] + [_around(k * s) for s in pick] + [SPECIALS] * 4)
    n = rows * cols
    if len(vals) > n:
        vals = rng.permutation(vals)[:n]
    x = np.concatenate([vals, (rng.standard_normal(n - len(vals)) * np.float32(40.0 * np.median(scales))).astype(np.float32)])
    rng.shuffle(x)
    return x.reshape(rows, cols).astype(np.float32)


def _planes(x, scales, lo, hi, rows_p, cols_p):
    """int8 [C][rows_p][cols_p], zero padded."""
    C = len(scales)
    out = np.zeros((C, rows_p, cols_p), np.int8)
    with np.errstate(all="ignore"):
        for c in range(C):
            out[c, :x.shape[0], :x.shape[1]] = _i8(_grid(x / np.float32(scales[c]), lo, hi))
    return out


def _frag_order(plane):
    """One [rows_p][cols_p] plane in the MFMA-fragment order of layout 3: the 16-byte chunk kc of row r goes to chunk
    ((((r / 64) * cols_p / 64 + kc / 4) * 2 + (r / 32) % 2) * 2 + (kc / 2) % 2) * 64 + (kc % 2) * 32 + r % 32."""
    rows_p, cols_p = plane.shape
    r, kc = np.meshgrid(np.arange(rows_p), np.arange(cols_p // 16), indexing="ij")
    chunk = ((((r // 64) * (cols_p // 64) + kc // 4) * 2 + (r // 32) % 2) * 2 + (kc // 2) % 2) * 64 + (kc % 2) * 32 + r % 32
    out = np.zeros((rows_p * cols_p // 16, 16), np.int8)
    out[chunk.reshape(-1)] = plane.reshape(rows_p, cols_p // 16, 16).reshape(-1, 16)
    return out.reshape(-1)


def _expected(planes, layout, live, before):
    """The destination after packing the candidates `live` (a boolean per candidate) of `planes` in `layout` over `before`."""
    C, rows_p, cols_p = planes.shape
    exp = before.copy()
    if layout == 0:
        v = exp.reshape(C, rows_p, cols_p)
        for c in np.flatnonzero(live):
            v[c] = planes[c]
    elif layout == 1:
        v = exp.reshape(rows_p, C, cols_p)
        for c in np.flatnonzero(live):
            v[:, c] = planes[c]
    elif layout == 2:
        v = exp.reshape(rows_p, (C + 1) // 2, cols_p // 64, 2, 64)
        for c in np.flatnonzero(live):
            v[:, c // 2, :, c % 2, :] = planes[c].reshape(rows_p, cols_p // 64, 64)
    else:
        assert live.sum() <= 1
        for c in np.flatnonzero(live):
            exp[:] = _frag_order(planes[c])
    return exp


def _size(C, layout, rows_p, cols_p):
    return rows_p * cols_p * (1 if layout == 3 else (C + 1) // 2 * 2 if layout == 2 else C)


def _run(eng, x, scales, layout, lo, hi, rows_p, crange=None, done=None, live_max=-1, general=False):
    cols_p = -(-x.shape[1] // 64) * 64
    out = torch.full((_size(len(scales), layout, rows_p, cols_p),), SENTINEL, dtype=torch.int8, device="cuda")
    cr = _t(np.asarray(crange, np.int32)) if crange is not None else None
    dn = _t(np.asarray(done, np.uint8)) if done is not None else None
    eng.debug_pack_cands(_t(x), _t(scales), layout=layout, lo=lo, hi=hi, rows_padded=rows_p, crange=cr, done=dn, live_max=live_max,
                         general=general, out=out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


GRIDS = [(8, 0.0123, False), (6, 0.0567, False), (8, 0.0123, True)]      # (bits, base scale, one scale with 1 / s = inf)
SHAPES = [(70, 256, 128), (37, 199, 64)]                                  # (rows, cols, rows_padded): aligned and ragged rows


@pytest.mark.parametrize("bit,base,overflow", GRIDS)
@pytest.mark.parametrize("rows,cols,rows_p", SHAPES)
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_all_candidates_match_ieee_division(eng, layout, rows, cols, rows_p, bit, base, overflow):
    q = 2 ** (bit - 1)
    lo, hi = -q, q - 1
    C = 23                                       # two full candidate groups and a partial one; odd: layout 2 pads the last pair
    scales = _scales(C, base, overflow)
    x = _source(rows, cols, scales, bit, seed=layout * 100 + rows + bit)
    cols_p = -(-cols // 64) * 64
    planes = _planes(x, scales, lo, hi, rows_p, cols_p)
    before = np.full(_size(C, layout, rows_p, cols_p), SENTINEL, np.int8)
    got = _run(eng, x, scales, layout, lo, hi, rows_p)
    np.testing.assert_array_equal(got, _expected(planes, layout, np.ones(C, bool), before))
    assert not planes[:, rows:, :].any() and not planes[:, :, cols:].any()


# device-side ranges over 37 candidates: empty, one candidate, straddling a multiple of ten, inside one group, everything,
# reaching past the table on either side (clipped)
RANGES = [(5, 5), (9, 4), (0, 1), (36, 37), (17, 18), (8, 13), (19, 31), (20, 30), (3, 9), (0, 37), (-4, 6), (30, 50)]


@pytest.mark.parametrize("a,b", RANGES)
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_pruned_range_packs_only_its_candidates(eng, layout, a, b):
    """Every byte outside the range keeps the sentinel; the launch that knows the length of the range, the one that knows an
    upper bound of it and the one that knows nothing write the same buffer."""
    C, rows, cols, rows_p, lo, hi = 37, 37, 199, 64, -128, 127
    scales = _scales(C, 0.0123)
    x = _source(rows, cols, scales, 8, seed=(a + 8) * 64 + b + layout)
    planes = _planes(x, scales, lo, hi, rows_p, 256)
    live = np.zeros(C, bool)
    live[max(a, 0):max(min(b, C), 0)] = True
    before = np.full(_size(C, layout, rows_p, 256), SENTINEL, np.int8)
    exp = _expected(planes, layout, live, before)
    n = int(live.sum())
    unknown = _run(eng, x, scales, layout, lo, hi, rows_p, crange=(a, b))
    np.testing.assert_array_equal(unknown, exp)
    for live_max in sorted({n, n + 1, n + 12, C}):
        known = _run(eng, x, scales, layout, lo, hi, rows_p, crange=(a, b), live_max=live_max)
        np.testing.assert_array_equal(known, exp, err_msg=f"live_max {live_max}")


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("bit", [8, 6])
def test_done_flags_mask_part_of_a_range(eng, layout, bit):
    q = 2 ** (bit - 1)
    C, rows, cols, rows_p, lo, hi = 37, 37, 199, 64, -q, q - 1
    scales = _scales(C, 0.0345)
    x = _source(rows, cols, scales, bit, seed=layout + bit)
    planes = _planes(x, scales, lo, hi, rows_p, 256)
    rng = np.random.default_rng(layout * 8 + bit)
    for a, b in [(4, 27), (10, 20), (0, 37)]:
        for done in (rng.integers(0, 2, C).astype(np.uint8), np.ones(C, np.uint8), np.zeros(C, np.uint8)):
            live = np.zeros(C, bool)
            live[a:b] = True
            live &= done == 0
            before = np.full(_size(C, layout, rows_p, 256), SENTINEL, np.int8)
            exp = _expected(planes, layout, live, before)
            np.testing.assert_array_equal(_run(eng, x, scales, layout, lo, hi, rows_p, crange=(a, b), done=done), exp)
            np.testing.assert_array_equal(_run(eng, x, scales, layout, lo, hi, rows_p, crange=(a, b), done=done, live_max=b - a), exp)


@pytest.mark.parametrize("bit", [8, 6])
@pytest.mark.parametrize("win", [0, 9, 10, 63, 99])
def test_one_candidate_of_a_range_in_fragment_order(eng, bit, win):
    """Stage B1 of a pruned pass: 100 candidates, a device-side range that holds the slice winner, ONE plane in fragment order;
    the host knows the length of the range, not where it lies."""
    q = 2 ** (bit - 1)
    C, rows, cols, rows_p, lo, hi = 100, 70, 199, 128, -q, q - 1
    scales = _scales(C, 0.0123)
    x = _source(rows, cols, scales, bit, seed=win + bit)
    plane = _planes(x, scales[win:win + 1], lo, hi, rows_p, 256)[0]
    exp = _frag_order(plane)
    np.testing.assert_array_equal(_run(eng, x, scales, 3, lo, hi, rows_p, crange=(win, win + 1)), exp)
    np.testing.assert_array_equal(_run(eng, x, scales, 3, lo, hi, rows_p, crange=(win, win + 1), live_max=1), exp)
    # an empty range packs nothing, a host that knows it to be empty launches nothing
    keep = np.full(rows_p * 256, SENTINEL, np.int8)
    np.testing.assert_array_equal(_run(eng, x, scales, 3, lo, hi, rows_p, crange=(win, win)), keep)
    np.testing.assert_array_equal(_run(eng, x, scales, 3, lo, hi, rows_p, crange=(win, win), live_max=0), keep)


@pytest.mark.parametrize("bit,s", [(8, 0.0123), (6, 0.0567), (8, 2.0e-39), (4, 0.31)])
@pytest.mark.parametrize("rows,cols,rows_p", [(70, 256, 128), (37, 199, 64), (64, 64, 64)])
@pytest.mark.parametrize("layout", [0, 1, 2, 3])
def test_single_plane_kernel(eng, layout, rows, cols, rows_p, bit, s):
    """k_pack1 against numpy's IEEE division and against k_pack with C = 1 (`general`), in every layout."""
    q = 2 ** (bit - 1)
    lo, hi = -q, q - 1
    scales = np.array([s], np.float32)
    x = _source(rows, cols, scales, bit, seed=rows + bit + layout)
    cols_p = -(-cols // 64) * 64
    planes = _planes(x, scales, lo, hi, rows_p, cols_p)
    exp = _expected(planes, layout, np.ones(1, bool), np.full(_size(1, layout, rows_p, cols_p), SENTINEL, np.int8))
    single = _run(eng, x, scales, layout, lo, hi, rows_p)
    general = _run(eng, x, scales, layout, lo, hi, rows_p, general=True)
    np.testing.assert_array_equal(single, exp)
    np.testing.assert_array_equal(general, exp)


@pytest.mark.parametrize("layout", [0, 1, 2, 3])
@pytest.mark.parametrize("bit", [8, 6])
def test_one_known_candidate_equals_the_general_kernel(eng, layout, bit):
    """A range the host knows to hold at most one candidate goes through k_pack1: same bytes as k_pack on the same range, with
    and without the candidate's `done` flag, and nothing where the range is empty."""
    q = 2 ** (bit - 1)
    C, rows, cols, rows_p, lo, hi = 37, 37, 199, 64, -q, q - 1
    scales = _scales(C, 0.0234, overflow=True)
    x = _source(rows, cols, scales, bit, seed=layout * 4 + bit)
    for a, b in [(0, 1), (18, 19), (36, 37), (36, 40), (-1, 1), (7, 7)]:
        for flag in (0, 1):
            done = np.zeros(C, np.uint8)
            done[max(a, 0)] = flag
            one = _run(eng, x, scales, layout, lo, hi, rows_p, crange=(a, b), done=done, live_max=1)
            ref = _run(eng, x, scales, layout, lo, hi, rows_p, crange=(a, b), done=done, live_max=1, general=True)
            np.testing.assert_array_equal(one, ref, err_msg=f"range [{a}, {b}) done {flag}")
            if flag or a == b:
                assert (one == SENTINEL).all()


def test_single_plane_padding_is_zero_for_any_scale(eng):
    """Rows and columns of padding are zero bytes even where 0 / s is not 0 (s = 0, NaN): as k_pack writes them."""
    rows, cols, rows_p = 37, 199, 64
    x = np.random.default_rng(5).standard_normal((rows, cols)).astype(np.float32)
    for s in (0.0, np.nan, np.inf):
        scales = np.array([s], np.float32)
        single = _run(eng, x, scales, 0, -128, 127, rows_p).reshape(rows_p, 256)
        general = _run(eng, x, scales, 0, -128, 127, rows_p, general=True).reshape(rows_p, 256)
        assert not single[rows:].any() and not single[:, cols:].any()
        np.testing.assert_array_equal(single, general)
        np.testing.assert_array_equal(single, _planes(x, scales, -128, 127, rows_p, 256)[0])
