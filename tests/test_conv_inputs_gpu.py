"""The encoder convolutions (csrc/convgemm.hip) on the GPU against the float64 oracle (tests/conv_oracle.py), on input
families with a scale, an offset, a dynamic range and impulses, through every launch form of the dispatch
(conv_oracle.CASES; tests/test_conv_host.py checks the list against the dispatch's rules).

The bound, for every cell (none is left out):   |got - want| <= E,   E = (3 * 2^-16 + 4 e(n) 2^-24) A   per layer, carried
through a stack by conv_oracle.stack_bound(); a cell with E == 0 (only zeros in reach, no bias) must be exactly 0.

Beside the bound: bias / ReLU combinations encode() never produces (straight through the C ABI), NaN and +inf
activations (a NaN covers its receptive field in all output channels and passes through ReLU; everything else keeps
the bits of the clean run; +inf is contained in the same field), a workspace full of zero or of 0xFF bytes (the same
bits), fenced buffers (stores stay inside; NaN around x and the bias never reaches a result), and the same bits call
after call and on a side stream."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import conv_oracle as C

pytestmark = pytest.mark.gpu

OPTIONS = (b"conv_narrow_ft", b"conv_split_always", b"conv_no_ring", b"conv_no_fuse")
FENCE, CANARY = 4096, 0xA5                                   # bytes of canary on either side
NAN_FENCE = 1024                                             # fp32 NaNs on either side of x and of a bias


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _reset():
    from aligner_amd import _lib
    lib = _lib.load()
    for name in OPTIONS:
        lib.aligner_debug_set_option(name, 0)


@pytest.fixture(autouse=True)
def options_reset(request):
    request.addfinalizer(_reset)


@contextlib.contextmanager
def forced(opts):
    from aligner_amd import _lib
    lib = _lib.load()
    try:
        for name, value in opts:
            assert lib.aligner_debug_set_option(name.encode(), value) == 0
        yield
    finally:
        _reset()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _device_layers(base, family):
    """The base case's weights and biases on the GPU, shared by its runs (the package keeps one prepared image each)."""
    dev = torch.device("cuda:0")
    _, layers = C.inputs(base, family)
    return [(torch.from_numpy(w).to(dev), None if b is None else torch.from_numpy(b).to(dev), relu) for w, b, relu in layers]


def _call(name, family, x=None):
    """One run of a case through aligner_amd.conv1d (one layer) or softattn.encode (a stack), its options in force."""
    import aligner_amd
    from aligner_amd.softattn import encode
    c = C.CASES[name]
    dev = torch.device("cuda:0")
    xd = torch.from_numpy(C.inputs(c.base, family)[0] if x is None else x).to(dev)
    layers = _device_layers(c.base, family)
    with forced(c.opts), torch.no_grad():
        if len(layers) == 1:
            w, b, relu = layers[0]
            y = aligner_amd.conv1d(xd, w, b, relu)
        else:
            y = encode(xd, [(w, b) for w, b, _ in layers])
        torch.cuda.synchronize()
    return y.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _run(name, family):
    """One GPU run per (case with its options, family), shared by the tests.  Never modified."""
    return _call(name, family)


# ---- inside the bound ----
@pytest.mark.parametrize("family", C.FAMILIES)
@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_every_cell_inside_the_bound(dev, name, family):
    c = C.CASES[name]
    _, _, want, E = C.reference(c.base, family)
    got = _run(name, family)
    assert got.shape == want.shape and got.dtype == np.float32
    r = C.ratio(got, want, E)
    zeros = int((E == 0).sum())
    print(f"{name:30s} {c.form:8s} {family:8s}: largest error / bound = {r:.3f}  ({zeros} cells with E = 0 are exact zeros)")
    if family == "impulse" and len(c.ks) == 1:
        assert zeros > 0
    assert r <= 1.0


# ---- straight through the C ABI: fenced buffers, a chosen workspace content, any bias / ReLU combination ----
class _Fenced:
    """nbytes of device memory, canary bytes before, inside and after."""

    def __init__(self, nbytes, dev, fill=None):
        self.n = int(nbytes)
        self.buf = torch.full((FENCE + self.n + (-self.n) % 256 + FENCE,), CANARY, dtype=torch.uint8, device=dev)
        if fill is not None:
            self.buf[FENCE:FENCE + self.n] = fill
        self.ptr = self.buf.data_ptr() + FENCE
        assert self.ptr % 256 == 0

    def intact(self):
        return bool((self.buf[:FENCE] == CANARY).all()) and bool((self.buf[FENCE + self.n:] == CANARY).all())

    def f32(self, shape):
        return self.buf[FENCE:FENCE + self.n].view(torch.float32).reshape(shape)


def _nan_fenced(a, dev, fenced):
    """fp32 data on the GPU, with NaNs on either side when fenced: (owner, pointer)."""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).reshape(-1)
    if not fenced:
        return t, t.data_ptr()
    buf = torch.full((2 * NAN_FENCE + t.numel(),), float("nan"), dtype=torch.float32, device=dev)
    buf[NAN_FENCE:NAN_FENCE + t.numel()] = t
    return buf, buf.data_ptr() + 4 * NAN_FENCE


def _raw(dev, x, layers, opts=(), ws_fill=None, nan_fences=False):
    """aligner_conv1d_prepared_ws_f32 (one layer) or aligner_conv_stack_f32 on layers [(w, b or None, relu)]: y, the
    workspace and the prepared images in canary-fenced allocations, x and the biases between NaNs when asked.  Returns
    (y as numpy, every fence intact)."""
    from aligner_amd import _lib
    lib = _lib.load()
    B, Cin, T = x.shape
    st = torch.cuda.current_stream(dev).cuda_stream
    keep, preps, biases = [], [], []
    for w, b, _ in layers:
        Cout, Ci, K = w.shape
        wd = torch.from_numpy(w).to(dev)
        n = lib.aligner_conv1d_prepared_bytes(Cout, Ci, K)
        assert n > 0
        p = _Fenced(n, dev)
        _lib.check(lib.aligner_conv1d_prepare_f32(wd.data_ptr(), p.ptr, n, Cout, Ci, K, st))
        bo, bp = (None, None) if b is None else _nan_fenced(b, dev, nan_fences)
        keep += [wd, bo]
        preps.append(p)
        biases.append(bp)
    xo, xp = _nan_fenced(x, dev, nan_fences)
    Cl = layers[-1][0].shape[0]
    y = _Fenced(4 * B * Cl * T, dev)
    with forced(opts):
        if len(layers) == 1:
            (w, _, relu), = layers
            Cout, _, K = w.shape
            nws = lib.aligner_conv1d_workspace_bytes(B, Cin, Cout, T, K)
            ws = _Fenced(nws, dev, ws_fill) if nws else None
            _lib.check(lib.aligner_conv1d_prepared_ws_f32(xp, preps[0].ptr, biases[0], y.ptr, ws.ptr if ws else None, nws,
                                                          B, Cin, Cout, T, K, int(relu), st))
        else:
            arr = (_lib.ConvLayer * len(layers))(*[_lib.ConvLayer(p.ptr, bp, w.shape[1], w.shape[0], w.shape[2], int(relu))
                                                   for p, bp, (w, _, relu) in zip(preps, biases, layers)])
            nws = lib.aligner_conv_stack_workspace_bytes(arr, len(layers), B, T)
            assert nws > 0, "this stack is meant to run as one call"
            ws = _Fenced(nws, dev, ws_fill)
            _lib.check(lib.aligner_conv_stack_f32(xp, arr, len(layers), y.ptr, ws.ptr, nws, B, T, st))
        torch.cuda.synchronize()
    intact = y.intact() and all(p.intact() for p in preps) and (ws is None or ws.intact())
    del keep, xo
    return y.f32((B, Cl, T)).cpu().numpy(), intact


F211 = (80, 160, 80, 80), (3, 1, 1)
COMBOS = {                                  # name: (chans, ks, layers with a bias, ReLU flags)
    "fused_no_bias_first": F211 + ((0, 1, 1), (1, 1, 0)),
    "fused_no_bias_middle": F211 + ((1, 0, 1), (1, 1, 0)),
    "fused_no_bias_last": F211 + ((1, 1, 0), (1, 1, 0)),
    "fused_relu_last": F211 + ((1, 1, 1), (1, 1, 1)),
    "fused_no_relu_between": F211 + ((1, 1, 1), (1, 0, 0)),
    "fused_no_bias_at_all_relu_last": F211 + ((0, 0, 0), (0, 1, 1)),
    "ring_relu_last_no_bias": ((128, 512, 33), (3, 1), (1, 0), (0, 1)),
    "wide_no_bias_relu": ((130, 130), (3,), (0,), (1,)),
    "narrow_no_bias_relu": ((33, 70), (5,), (0,), (1,)),
    "none_no_bias_relu": ((8, 40), (3,), (0,), (1,)),
}


@pytest.mark.parametrize("family", ["unit", "wide", "impulse"])
@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_bias_and_relu_combinations_through_the_c_abi(dev, combo, family):
    """What encode() never produces: a NULL bias in the first, a middle and the last layer of a fused stack, ReLU on the
    last layer, no ReLU between two fused layers -- the same bound."""
    chans, ks, has_bias, relus = COMBOS[combo]
    B, T = 2, 70
    rng = np.random.default_rng(C._seed(combo, family))
    x = C.draw(family, rng, (B, chans[0], T))
    layers = []
    for ci, co, k, hb, relu in zip(chans[:-1], chans[1:], ks, has_bias, relus):
        w, b = C.draw_weights(rng, co, ci, k)
        layers.append((w, b if hb else None, bool(relu)))
    hs, Es = C.stack_bound(x, layers)
    got, intact = _raw(dev, x, layers)
    r = C.ratio(got, hs[-1], Es[-1])
    print(f"{combo:32s} {family:8s}: largest error / bound = {r:.3f}")
    assert intact
    assert r <= 1.0


# ---- non-finite activations ----
NONFINITE_CASES = ("none_8_40_k3", "none_64_300_k5", "wide_130_130_k3", "wide_160_256_k5", "narrow_80_160_k3",
                   "narrow_80_80_k1_split", "ring_128_512_33", "fused211_T130", "mixed_k5331", "mixed_wide_ring_fused")


def _place(c, where):
    Cin, T = c.chans[0], c.T
    if where == "first":
        return 0, 0, 0
    if where == "last":
        return 0, Cin - 1, T - 1
    edge = 128 if T > 129 else 16                              # a frame-tile edge, from either side
    return 1, Cin // 2, edge - (len(c.ks) > 1)


@pytest.mark.parametrize("where", ["first", "last", "edge"])
@pytest.mark.parametrize("name", NONFINITE_CASES)
def test_a_nan_covers_its_receptive_field_and_nothing_else(dev, name, where):
    """One NaN activation: isnan(got) == isnan(float64 reference) exactly -- its receptive field, all output channels,
    through every ReLU (torch.relu keeps NaN) --, every other cell with the bits of the clean run."""
    c = C.CASES[name]
    x, layers = C.inputs(c.base, "unit")
    x = x.copy()
    x[_place(c, where)] = np.nan
    want_nan = np.isnan(C.encode64(x, layers))
    got, clean = _call(name, "unit", x), _run(name, "unit")
    got_nan = np.isnan(got)
    print(f"{name} {where}: {int(want_nan.sum())} NaN cells expected, {int(got_nan.sum())} found, "
          f"{int((want_nan & ~got_nan).sum())} lost, {int((got_nan & ~want_nan).sum())} stray")
    assert want_nan.any() and not np.isnan(clean).any()
    assert np.array_equal(got_nan, want_nan)
    assert np.array_equal(_bits(got)[~want_nan], _bits(clean)[~want_nan])


@pytest.mark.parametrize("where", ["first", "last", "edge"])
@pytest.mark.parametrize("name", NONFINITE_CASES)
def test_an_inf_stays_inside_its_receptive_field(dev, name, where):
    """+inf activations come out as NaN (split_bf16: lo = inf - inf; include/aligner_amd.h says so), so containment only:
    outside the planted value's receptive field the clean run's bits, inside it non-finite or equal to the reference."""
    c = C.CASES[name]
    x, layers = C.inputs(c.base, "unit")
    x = x.copy()
    at = _place(c, where)
    x[at] = np.nan
    field = np.isnan(C.encode64(x, layers))
    x[at] = np.inf
    want = C.encode64(x, layers)
    assert np.isfinite(want[~field]).all()
    got, clean = _call(name, "unit", x), _run(name, "unit")
    assert np.array_equal(_bits(got)[~field], _bits(clean)[~field])
    with np.errstate(invalid="ignore"):
        assert (~np.isfinite(got[field]) | (got[field] == want[field].astype(np.float32))).all()


# ---- the workspace's previous contents ----
WORKSPACE_CASES = tuple(n for n in C.CASE_NAMES if n.startswith("wide_") or n.endswith("_split")) + (
    "ring_128_512_33", "mixed_wide_ring_fused")


@pytest.mark.parametrize("name", WORKSPACE_CASES)
def test_the_workspace_contents_before_the_call_do_not_matter(dev, name):
    """The same call on a workspace of zero bytes and on one of 0xFF bytes (every bf16 and fp32 pattern a NaN): the same
    output bits, no NaN."""
    c = C.CASES[name]
    x, layers = C.inputs(c.base, "unit")
    y0, ok0 = _raw(dev, x, layers, c.opts, ws_fill=0x00)
    y1, ok1 = _raw(dev, x, layers, c.opts, ws_fill=0xFF)
    assert ok0 and ok1
    assert not np.isnan(y1).any()
    assert np.array_equal(_bits(y0), _bits(y1))
    assert np.array_equal(_bits(y0), _bits(_run(name, "unit")))


# ---- loads and stores stay inside their buffers ----
FENCE_CASES = ("none_8_40_k3", "none_64_300_k5", "wide_128_128_k1", "wide_130_130_k3", "wide_160_256_k5", "narrow_33_70_k5",
               "narrow_80_160_k3_ft8", "narrow_80_80_k1_split", "narrow_1024_80_k1", "ring_128_512_33", "fused211_T70",
               "fused211_T130", "mixed_k5331")


@pytest.mark.parametrize("name", FENCE_CASES)
def test_loads_and_stores_stay_inside_their_buffers(dev, name):
    """y, the workspace and the prepared images between canary bytes (intact afterwards, no output element left as
    canary); x and the biases between NaNs: an out-of-range read that reaches a result would show, the result has the
    bits of the run on the package's own allocations."""
    c = C.CASES[name]
    x, layers = C.inputs(c.base, "unit")
    got, intact = _raw(dev, x, layers, c.opts, nan_fences=True)
    assert intact
    assert not (_bits(got) == 0xA5A5A5A5).any()
    assert np.array_equal(_bits(got), _bits(_run(name, "unit")))


# ---- the same bits, call after call and on a side stream ----
@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_two_calls_give_the_same_bits(dev, name):
    family = "wide"
    assert np.array_equal(_bits(_call(name, family)), _bits(_run(name, family)))


@pytest.mark.parametrize("name", ["wide_130_130_k3", "narrow_80_160_k3", "none_8_40_k3", "ring_128_512_33", "fused211_T130",
                                  "mixed_wide_ring_fused"])
def test_on_a_side_stream(dev, name):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    c = C.CASES[name]
    x, layers = C.inputs(c.base, "unit")
    with torch.cuda.stream(side):
        got = _call(name, "unit")
        raw, intact = _raw(dev, x, layers, c.opts)
    side.synchronize()
    assert np.array_equal(_bits(got), _bits(_run(name, "unit")))
    assert intact and np.array_equal(_bits(raw), _bits(got))
