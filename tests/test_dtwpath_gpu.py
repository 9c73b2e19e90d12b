"""Hard DTW on the GPU (aligner_amd/dtwpath.py, csrc/dtwpath.hip): value, path and length against the NumPy float32
restatement of tests/dtwpath_oracle.py bit for bit -- no tolerance anywhere -- in dense and in band storage (the oracle
has the cases and says which kernel edges they straddle); band storage against the dense call; special values; the
validity of the GPU's own path; infeasible utterances; determinism; guard bands; want_path=False; dtw_path_l1."""
import functools

import numpy as np
import pytest
import torch

import banddtw_oracle as bo
import dtwpath_oracle as dpo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _i32(t, dev):
    return None if t is None else torch.tensor(t, dtype=torch.int32, device=dev)


def _np(r):
    torch.cuda.synchronize()
    return tuple(None if x is None else x.cpu().numpy() for x in r)


def _call(c, cost, dev, **kw):
    """The case's call on a cost table [B,N,M] (numpy): dense, or in band storage for a band case."""
    import aligner_amd
    if c.name in dpo.BAND_NAMES:
        band = torch.tensor(bo.to_band(np.asarray(cost), c.w)).to(dev)
        return aligner_amd.dtw_path_banded(band, _i32(c.n, dev), _i32(c.m, dev), c.p, **kw)
    return aligner_amd.dtw_path(torch.tensor(np.asarray(cost)).to(dev), _i32(c.n, dev), _i32(c.m, dev), c.p, c.w, **kw)


@functools.lru_cache(maxsize=None)
def _run(name):
    """One GPU run per case, shared by the tests: (value [B], path [B,L,2], length [B]) as numpy arrays."""
    c, cost, *_ = dpo.reference(name)
    return _np(_call(c, cost, torch.device("cuda:0")))


def _same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize("name", dpo.DENSE_NAMES + dpo.BAND_NAMES)
def test_value_path_and_length_have_the_oracles_bits(dev, name):
    c, cost, value, path, length = dpo.reference(name)
    got = _run(name)
    assert got[1].shape == (c.B, c.L, 2)
    for b in range(c.B):
        if not _same([g[b] for g in got], [value[b], path[b], length[b]]):
            K = int(min(got[2][b], length[b]))
            diff = np.nonzero((got[1][b, :K] != path[b, :K]).any(axis=1))[0]
            print(f"{name}[{b}]: value {got[0][b]!r} / {value[b]!r}, length {got[2][b]} / {length[b]}, first differing step "
                  f"{diff[:1]}: {got[1][b, diff[:1]]} / {path[b, diff[:1]]}")
    assert _same(got, (value, path, length))


@pytest.mark.parametrize("name", [n for n in dpo.BAND_NAMES if dpo.CASES[n].N <= 1024])
def test_band_storage_has_the_dense_calls_bits(dev, name):
    """dtw_path_banded equals dtw_path on band_to_dense(..., fill=+inf) with bandwidth w in all three outputs (the path
    buffers differ in length: compared up to the shorter, the rest is -1)."""
    import aligner_amd
    c, cost, *_ = dpo.reference(name)
    value, path, length = _run(name)
    band = torch.tensor(bo.to_band(cost, c.w)).to(dev)
    dense = aligner_amd.band_to_dense(band, c.M, fill=float("inf"))
    v, p, k = _np(aligner_amd.dtw_path(dense, _i32(c.n, dev), _i32(c.m, dev), c.p, c.w))
    L = min(p.shape[1], path.shape[1])
    assert v.tobytes() == value.tobytes() and np.array_equal(k, length)
    assert np.array_equal(p[:, :L], path[:, :L]) and (p[:, L:] == -1).all() and (path[:, L:] == -1).all()


@pytest.mark.parametrize("name", ["d100x127_w30_ragged", "d64x64_w0", "band_ragged", "band_w64", "band_wide", "band_steps32"])
def test_nan_or_inf_where_no_cell_exists_changes_no_bit(dev, name):
    c, cost, *_ = dpo.reference(name)
    ns, ms = dpo.lengths_of(c)
    i, j = np.mgrid[0:c.N, 0:c.M]
    exists = (i[None] < ns[:, None, None]) & (j[None] < ms[:, None, None]) & (np.abs(i - j)[None] <= c.w)
    for fill in (np.nan, np.inf):
        bad = np.where(exists, cost, np.float32(fill))
        if c.name in dpo.BAND_NAMES:                              # elements of band storage whose column is outside [0, M) as well
            import aligner_amd
            band = bo.to_band(bad, c.w, fill)
            got = _np(aligner_amd.dtw_path_banded(torch.tensor(band).to(dev), _i32(c.n, dev), _i32(c.m, dev), c.p))
        else:
            got = _np(_call(c, bad, dev))
        assert _same(got, _run(name)), fill


@pytest.mark.parametrize("name", ["d65x80", "band_w31"])
def test_a_nan_cost_is_a_forbidden_cell_and_minus_inf_propagates(dev, name):
    c, cost, value, path, length = dpo.reference(name)
    on = [tuple(x) for x in path[0, :length[0]]]
    cell = on[len(on) // 2]                                       # a cell of utterance 0's optimal path
    a, b = cost.copy(), cost.copy()
    a[0][cell] = np.nan
    b[0][cell] = np.inf
    got_nan, got_inf = _np(_call(c, a, dev)), _np(_call(c, b, dev))
    assert _same(got_nan, got_inf) and _same(got_inf, dpo.dtw_path32(b, c.n, c.m, c.p, c.w, c.L))
    assert cell not in [tuple(x) for x in got_nan[1][0, :got_nan[2][0]]]
    assert _same([g[1] for g in got_nan], [g[1] for g in _run(name)])          # the other utterance: no bit changed
    off = next((i, j) for i in range(5, c.N) for j in range(c.M) if (c.w is None or abs(i - j) <= c.w) and (i, j) not in on)
    d = cost.copy()
    d[0][off] = -np.inf
    got = _np(_call(c, d, dev))
    assert _same(got, dpo.dtw_path32(d, c.n, c.m, c.p, c.w, c.L))
    assert got[0][0] == -np.inf and off in [tuple(x) for x in got[1][0, :got[2][0]]]
    dpo.check_path(got[1][0], got[2][0], c.N, c.M, c.w, d[0])


@pytest.mark.parametrize("name", dpo.DENSE_NAMES + dpo.BAND_NAMES)
def test_the_gpus_path_is_a_warping_path_and_adds_up_to_the_value(dev, name):
    c, cost, *_ = dpo.reference(name)
    value, path, length = _run(name)
    ns, ms = dpo.lengths_of(c)
    worst = 0.0
    for b in range(c.B):
        n, m = int(ns[b]), int(ms[b])
        if value[b] == np.inf:
            assert length[b] == 0 and (path[b] == -1).all()
            continue
        dpo.check_path(path[b], length[b], n, m, c.w, cost[b])
        total, S = dpo.path_sums(cost[b], path[b], length[b], c.p)
        err, bound = abs(float(value[b]) - total), dpo.value_bound(n, m, S)
        worst = max(worst, err / bound if bound else float(err > 0))
        print(f"{name}[{b}] n={n} m={m} K={length[b]}: |value - sum over the path| {err:.3e} / bound {bound:.3e}")
        assert err <= bound
    print(f"{name}: largest observed / bound {worst:.4f}")


def test_infeasible_utterances_leave_their_neighbours_alone(dev):
    for name in ("d100x127_w30_ragged", "band_ragged"):
        c, cost, *_ = dpo.reference(name)
        value, path, length = _run(name)
        assert (value[4:] == np.inf).all() and not length[4:].any() and (path[4:] == -1).all()
        assert np.isfinite(value[:4]).all() and (length[:4] > 0).all()
        keep = [0, 1, 2, 3]
        sub = type(c)(**{**vars(c), "B": 4, "n": tuple(c.n[k] for k in keep), "m": tuple(c.m[k] for k in keep)})
        assert _same(_np(_call(sub, cost[keep], dev)), (value[keep], path[keep], length[keep]))
    value, path, length = _run("forbidden")                        # +inf costs across every path of utterance 1
    assert value[1] == np.inf and length[1] == 0 and (path[1] == -1).all() and np.isfinite(value[0])


def test_two_runs_give_the_same_bits_and_want_path_false_the_same_value(dev):
    for name in ("d130x70_p", "ints65x80", "band_ragged", "band_w127", "band_past1024"):
        c, cost, *_ = dpo.reference(name)
        again = _np(_call(c, cost, dev))
        assert _same(again, _run(name))
        value, none, none2 = _call(c, cost, dev, want_path=False)
        torch.cuda.synchronize()
        assert none is None and none2 is None and value.cpu().numpy().tobytes() == again[0].tobytes()


def test_empty_shapes_and_half_precision(dev):
    import aligner_amd
    r = aligner_amd.dtw_path(torch.zeros(2, 0, 5, device=dev))
    assert torch.isinf(r.value).all() and r.path.shape == (2, 4, 2) and not r.length.any()
    r = aligner_amd.dtw_path_banded(torch.zeros(0, 4, 5, device=dev))
    assert r.value.shape == (0,) and r.path.shape == (0, 9, 2)
    c, cost, *_ = dpo.reference("d65x80")
    half = torch.tensor(cost).to(dev).to(torch.bfloat16)
    got = _np(aligner_amd.dtw_path(half.transpose(1, 2).contiguous().transpose(1, 2)))         # not contiguous, bf16
    assert _same(got, dpo.dtw_path32(half.float().cpu().numpy()))


# ---- guard bands ----------------------------------------------------------------------------------------------------------

FENCE, CANARY = 4096, 0xA5                                      # bytes of canary on either side


def _fenced(nbytes, dev):
    buf = torch.full((FENCE + nbytes + (-nbytes) % 256 + FENCE,), CANARY, dtype=torch.uint8, device=dev)
    return buf, buf.data_ptr() + FENCE


def _intact(buf, nbytes):
    return bool((buf[:FENCE] == CANARY).all()) and bool((buf[FENCE + nbytes:] == CANARY).all())


@pytest.mark.parametrize("name", ["d1x1", "d1x40", "d40x1", "d65x80", "d130x70_p", "d100x127_w30_ragged", "d1024x1030_w40",
                                  "band_w0", "band_w63", "band_w64", "band_wide", "band_ragged", "band_steps31",
                                  "band_steps32", "band_past1024"])
def test_stores_stay_inside_their_buffers(dev, name):
    """value, path, length and the workspace carved out of canary-filled allocations, the C ABI called on the interior
    pointers: nothing outside them is written, and what is inside has the oracle's bits."""
    from aligner_amd import _lib
    lib = _lib.load()
    c, cost, *_ = dpo.reference(name)
    banded = name in dpo.BAND_NAMES
    table = torch.tensor(bo.to_band(cost, c.w) if banded else cost).to(dev)
    nws = lib.aligner_dtw_path_banded_workspace_bytes(c.B, c.N, c.w) if banded else lib.aligner_dtw_path_workspace_bytes(c.B, c.N, c.M)
    assert nws >= table.numel()
    sizes = dict(value=4 * c.B, path=8 * c.B * c.L, length=4 * c.B, ws=nws)
    bufs = {k: _fenced(v, dev) for k, v in sizes.items()}
    n, m = _i32(c.n, dev), _i32(c.m, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    head = (table.data_ptr(), None if n is None else n.data_ptr(), None if m is None else m.data_ptr(), c.p)
    tail = (bufs["value"][1], bufs["path"][1], bufs["length"][1], bufs["ws"][1], nws, c.B, c.N)
    if banded:
        _lib.check(lib.aligner_dtw_path_banded_f32(*head, c.w, *tail, stream))
    else:
        _lib.check(lib.aligner_dtw_path_f32(*head, -1 if c.w is None else c.w, *tail, c.M, stream))
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        assert _intact(buf, sizes[k]), k
    got = tuple(bufs[k][0][FENCE:FENCE + sizes[k]].view(dt).reshape(shape).cpu().numpy()
                for k, dt, shape in (("value", torch.float32, (c.B,)), ("path", torch.int32, (c.B, c.L, 2)), ("length", torch.int32, (c.B,))))
    assert _same(got, _run(name))
    # without a path: the value alone, and not a byte of the path, the length or the workspace
    fresh = {k: _fenced(v, dev) for k, v in sizes.items()}
    tail = (fresh["value"][1], None, None, None, 0, c.B, c.N)
    if banded:
        _lib.check(lib.aligner_dtw_path_banded_f32(*head, c.w, *tail, stream))
    else:
        _lib.check(lib.aligner_dtw_path_f32(*head, -1 if c.w is None else c.w, *tail, c.M, stream))
    torch.cuda.synchronize()
    assert fresh["value"][0][FENCE:FENCE + 4 * c.B].view(torch.float32).cpu().numpy().tobytes() == got[0].tobytes()
    assert _intact(fresh["value"][0], sizes["value"])


def test_c_abi_error_codes(dev):
    from aligner_amd import _lib
    lib = _lib.load()
    x = torch.zeros(4096, device=dev)
    p = x.data_ptr()
    assert lib.aligner_dtw_path_f32(None, None, None, 0.0, -1, p, p, p, p, 1 << 20, 1, 4, 4, None) == _lib.EINVAL
    assert lib.aligner_dtw_path_f32(p, None, None, 0.0, -1, p, p, None, p, 1 << 20, 1, 4, 4, None) == _lib.EINVAL
    assert lib.aligner_dtw_path_f32(p, None, None, -1.0, -1, p, p, p, p, 1 << 20, 1, 4, 4, None) == _lib.EINVAL
    assert lib.aligner_dtw_path_f32(p, None, None, 0.0, -1, p, p, p, p, 1 << 20, 1, 1025, 4, None) == _lib.EDOM
    assert lib.aligner_dtw_path_f32(p, None, None, 0.0, -1, p, p, p, p, 15, 1, 4, 4, None) == _lib.ENOSPC
    assert lib.aligner_dtw_path_banded_f32(p, None, None, 0.0, 128, p, p, p, p, 1 << 20, 1, 4, None) == _lib.EDOM
    assert lib.aligner_dtw_path_banded_f32(p, None, None, float("inf"), 2, p, p, p, p, 1 << 20, 1, 4, None) == _lib.EINVAL
    assert lib.aligner_dtw_path_banded_f32(p, None, None, 0.0, 2, p, p, p, p, 19, 1, 4, None) == _lib.ENOSPC
    assert lib.aligner_dtw_path_workspace_bytes(1, 1025, 4) == 0 and lib.aligner_dtw_path_banded_workspace_bytes(1, 4, 128) == 0


@pytest.mark.parametrize("bandwidth", [20, None])
def test_dtw_path_l1_is_its_two_parts(dev, bandwidth):
    """[2,8,65,80]: l1_cost_banded + dtw_path_banded at w = 20, l1_cost + dtw_path without a band; and the evaluation
    recipe of the docstring adds up to the value."""
    import aligner_amd
    rng = np.random.default_rng(8)
    pred = torch.tensor(rng.uniform(-1, 1, (2, 8, 65)).astype(np.float32)).to(dev)
    target = torch.tensor(rng.uniform(-1, 1, (2, 8, 80)).astype(np.float32)).to(dev)
    n, m = _i32((65, 50), dev), _i32((80, 61), dev)
    got = aligner_amd.dtw_path_l1(pred, target, n, m, 0.1, bandwidth, 1.0 / 8)
    if bandwidth is None:
        cost = aligner_amd.l1_cost(pred, target, n, m, None, 1.0 / 8)
        want = aligner_amd.dtw_path(cost, n, m, 0.1)
        assert got.path.shape == (2, 65 + 80 - 1, 2)
    else:
        band = aligner_amd.l1_cost_banded(pred, target, n, m, bandwidth, 1.0 / 8)
        want = aligner_amd.dtw_path_banded(band, n, m, 0.1)
        cost = aligner_amd.band_to_dense(band, 80)
        assert got.path.shape == (2, 2 * 65 + bandwidth - 1, 2)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and torch.isfinite(got.value).all()
    for b in range(2):
        ij = got.path[b, :got.length[b]].long()
        stalls = int(((ij[1:] - ij[:-1]).sum(1) == 1).sum())
        on = float(cost[b, ij[:, 0], ij[:, 1]].double().sum())
        assert abs(on + 0.1 * stalls - float(got.value[b])) <= dpo.value_bound(65, 80, on + 0.1 * len(ij))
