"""Float64 restatement of the encoder convolutions (aligner_amd.conv1d, aligner_amd.softattn.encode), for the tests of
csrc/convgemm.hip: tests/test_conv_host.py (derivations, no GPU) and tests/test_conv_inputs_gpu.py.

    y[b,o,t] = act(bias[o] + sum_{i,k} w[o,i,k] x[b,i,t+k-K/2]),    zero padded ("same"), K in {1,3,5}, layout [B,C,T]

on the fp32 input values, and beside it what a relative error of the products is relative to,

    A[b,o,t] = |bias[o]| + sum_{i,k} |w[o,i,k]| |x[b,i,t+k-K/2]|                                 (magnitude())

The bound of one layer, per cell:      E = c(Cin, K) A,     c = 3 * 2^-16 + 4 e(n) 2^-24,   n = Cin K      (coeff())

3 * 2^-16 is the worst case of one split product (softattn_oracle64.split_bound's derivation: x = hi + lo + r with
|lo| <= 2^-8 |x|, |r| <= 2^-16 |x|; hi*hi + hi*lo + lo*hi misses lo*lo and the two r terms), which holds for any input and
any fan-in; e(n) 2^-24 A is what an fp32 product-and-add chain over the n terms loses (E_TABLE, measured by
simulate_fp32_chain over every input family: tests/test_conv_host.py keeps the table honest), times 4 for the matrix
cores' unknown accumulation order.

A stack: ReLU is 1-Lipschitz, so with h the float64 activations and E_0 = 0

    E_l = c_l A_l + |W_l| (*) E_{l-1},      A_l = magnitude(|h_{l-1}| + E_{l-1}, W_l, b_l)                (stack_bound())

simulate_split / simulate_fp32_chain restate the kernels' two sources of error one at a time (three bf16 split products
accumulated exactly / exact products accumulated in fp32)."""
import collections
import functools
import zlib

import numpy as np

from softattn_oracle64 import bf16


def _f64(x):
    """fp32 operands -> their values in float64; float64 arrays (a stack's activations, magnitudes) as they are."""
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    x = np.asarray(x)
    return x if x.dtype == np.float64 else x.astype(np.float32).astype(np.float64)


def _conv(x, w):
    """sum_{i,k} w[o,i,k] x[b,i,t+k-K/2] on float64 arrays (no conversion: also used on magnitudes and bounds)."""
    B, Cin, T = x.shape
    Cout, Cin2, K = w.shape
    assert Cin2 == Cin and K in (1, 3, 5)
    h = K // 2
    xp = np.zeros((B, Cin, T + 2 * h))
    xp[:, :, h:h + T] = x
    y = np.zeros((B, Cout, T))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(K):
            y += np.matmul(w[None, :, :, k], xp[:, :, k:k + T])
    return y


def conv64(x, w, b, relu):
    """x [B,Cin,T], w [Cout,Cin,K], b [Cout] or None -> [B,Cout,T] float64.  ReLU is np.maximum: NaN passes."""
    x, w = _f64(x), _f64(w)
    y = _conv(x, w)
    if b is not None:
        y = y + _f64(b)[None, :, None]
    return np.maximum(y, 0.0) if relu else y


def encode64(x, layers, every=False):
    """layers: [(w, b or None, relu)].  The last layer's output, or with every=True the list of every layer's."""
    h, out = _f64(x), []
    for w, b, relu in layers:
        h = conv64(h, w, b, relu)
        out.append(h)
    return out if every else h


def magnitude(x_abs, w, b):
    """A[b,o,t] = |bias[o]| + sum |w[o,i,k]| |x[b,i,t+k-K/2]|; x_abs float64, taken as it is (a stack adds its bound)."""
    a = _conv(np.abs(np.asarray(x_abs, np.float64)), np.abs(_f64(w)))
    return a if b is None else a + np.abs(_f64(b))[None, :, None]


SPLIT = 3 * 2.0 ** -16
# e(n): max |simulate_fp32_chain - conv64| / A in units of 2^-24 per (Cin, K), over every layer of CASES with that key,
# every input family and both weight families, rounded up (tests/test_conv_host.py: covers the simulation, at most twice it)
E_TABLE = {(8, 3): 5.5, (12, 1): 4.7, (16, 3): 8.0, (33, 5): 11.0, (40, 5): 10.0, (48, 3): 4.6, (48, 5): 8.4, (64, 1): 10.5, (64, 3): 10.0,
           (64, 5): 10.5, (80, 1): 9.5, (80, 3): 19.5, (96, 1): 7.8, (128, 1): 12.0, (128, 3): 12.0, (130, 1): 4.5,
           (130, 3): 20.0, (160, 1): 5.0, (160, 5): 11.0, (512, 1): 5.7, (1024, 1): 9.5}


def coeff(Cin, K):
    return SPLIT + 4 * E_TABLE[(Cin, K)] * 2.0 ** -24


def layer_bound(x, w, b, E_in=None):
    """(A, E) of one layer on the float64 activations x whose own error is at most E_in per cell."""
    x = _f64(x) if E_in is None else x
    A = magnitude(np.abs(x) + (0.0 if E_in is None else E_in), w, b)
    E = coeff(w.shape[1], w.shape[2]) * A
    if E_in is not None:
        E = E + _conv(E_in, np.abs(_f64(w)))
    return A, E


def stack_bound(x, layers):
    """([h_l], [E_l]): the float64 activations after every layer and the bound on the kernels' error in them."""
    h, E, hs, Es = _f64(x), None, [], []
    for w, b, relu in layers:
        _, E = layer_bound(h, w, b, E_in=np.zeros_like(h) if E is None else E)
        h = conv64(h, w, b, relu)
        hs.append(h)
        Es.append(E)
    return hs, Es


def simulate_split(x, w, b, K, drop=()):
    """The layer before its activation with the kernels' three split products -- hi = bf16(v), lo = bf16(v - hi);
    "hh" = x.hi w.hi, "hl" = x.hi w.lo, "lh" = x.lo w.hi -- accumulated exactly (float64), plus the bias.  `drop` leaves
    products out (for the tests of the tests)."""
    x, w = _f64(x), _f64(w)
    assert w.shape[2] == K
    xh, wh = bf16(x), bf16(w)
    xl, wl = bf16(x - xh), bf16(w - wh)
    y = np.zeros((x.shape[0], w.shape[0], x.shape[2]))
    for name, a, c in (("hh", xh, wh), ("hl", xh, wl), ("lh", xl, wh)):
        if name not in drop:
            y += _conv(a, c)
    return y if b is None else y + _f64(b)[None, :, None]


def simulate_fp32_chain(x, w, b):
    """The layer before its activation as an np.float32 product-and-add chain over the n = Cin K terms (input channel
    outermost, as the kernels' chunks), the bias added last; float64 of the result."""
    x32, w32 = np.asarray(_f64(x), np.float32), np.asarray(_f64(w), np.float32)
    B, Cin, T = x32.shape
    Cout, _, K = w32.shape
    h = K // 2
    xp = np.zeros((B, Cin, T + 2 * h), np.float32)
    xp[:, :, h:h + T] = x32
    acc = np.zeros((B, Cout, T), np.float32)
    for i in range(Cin):
        for k in range(K):
            acc += w32[None, :, i, k, None] * xp[:, None, i, k:k + T]
    if b is not None:
        acc += np.asarray(_f64(b), np.float32)[None, :, None]
    return acc.astype(np.float64)


# ---- inputs ----
FAMILIES = ("unit", "offset3", "scale30", "small", "relu", "wide", "impulse")
IMPULSE_CHANNELS = (0, 7, 8, 31, 32)                       # and Cin - 1
IMPULSE_FRAMES = (0, 1, 15, 16, 63, 64, 127, 128, 207, 208)    # and T - 1


def impulse_places(B, C, T):
    """[(b, c, t)] of the `impulse` family: the frames dealt round robin to the utterances (each gets another subset), the
    channels walked along with them."""
    cs = sorted({c for c in IMPULSE_CHANNELS + (C - 1,) if c < C})
    ts = sorted({t for t in IMPULSE_FRAMES + (T - 1,) if t < T})
    return [(j % B, cs[(j + j // len(cs)) % len(cs)], t) for j, t in enumerate(ts)]


def draw(family, rng, shape):
    """fp32 activations [B,C,T] of one input family."""
    n = rng.standard_normal(shape)
    if family == "unit":
        x = n
    elif family == "offset3":
        x = 3.0 + n
    elif family == "scale30":
        x = 30.0 * n
    elif family == "small":
        x = 0.01 * n
    elif family == "relu":
        x = 2.0 * np.abs(n)
    elif family == "wide":
        x = n * 10.0 ** rng.uniform(-3.0, 2.0, shape)
    elif family == "impulse":
        x = np.zeros(shape)
        for b, c, t in impulse_places(*shape):
            x[b, c, t] = 1.0
    else:
        raise ValueError(family)
    return x.astype(np.float32)


def draw_weights(rng, Cout, Cin, K, wide=False):
    w = rng.standard_normal((Cout, Cin, K)) / np.sqrt(Cin * K)
    if wide:
        w = w * 10.0 ** rng.uniform(-3.0, 2.0, w.shape)
    return w.astype(np.float32), rng.standard_normal(Cout).astype(np.float32)


# ---- the cases: the smallest shapes that reach every launch form of conv_plan / conv_launch / fused_plan ----
# form: what the dispatch is expected to do with the case (expected_form() restates the channel rules; the host test
# compares): "none" | "wide8" | "wide13" | "narrow" for one layer, "ring" / "fused<key>" / "chain" for a stack.
# opts: debug options (aligner_debug_set_option) in force during the run.  relu: of a single layer (a stack has ReLU
# between its layers and none at the end, as encode() runs it).  wide_w: weights with the `wide` per-element factor.
Case = collections.namedtuple("Case", "name B T chans ks relu form opts wide_w base")


def _case(name, B, T, chans, ks, relu=False, form="", opts=(), wide_w=False, base=None):
    return Case(name, B, T, tuple(chans), tuple(ks), relu, form, tuple(opts), wide_w, base or name)


def _cases():
    out = [
        # no GEMM form (conv1d_prepared_kernel)
        _case("none_8_40_k3", 2, 70, (8, 40), (3,), True, "none"),             # Cin < 16, 64-frame grid, T crosses 64
        _case("none_64_300_k5", 2, 130, (64, 300), (5,), False, "none"),       # Cout > 256 with Cin < 128, 128-frame grid
        _case("none_12_40_k1_T72", 2, 72, (12, 40), (1,), True, "none"),        # T % 4 == 0: the input read as aligned quads
        # wide
        _case("wide_128_128_k1", 2, 16, (128, 128), (1,), False, "wide8"),     # the smallest shape
        _case("wide_130_130_k3", 2, 201, (130, 130), (3,), True, "wide13"),    # ragged channels, scalar stores
        _case("wide_160_256_k5", 2, 300, (160, 256), (5,), False, "wide8"),    # three frame tiles, two halo frames
        _case("wide_128_128_k1_T410", 1, 410, (128, 128), (1,), True, "wide13"),   # two frame tiles
        _case("wide_130_130_k3_ww", 2, 201, (130, 130), (3,), True, "wide13", wide_w=True),
        # narrow, staged from fp32
        _case("narrow_80_80_k1", 2, 333, (80, 80), (1,), False, "narrow"),     # NT = 1
        _case("narrow_80_160_k3", 2, 130, (80, 160), (3,), True, "narrow"),    # NT = 2
        _case("narrow_33_70_k5", 2, 129, (33, 70), (5,), True, "narrow"),
        _case("narrow_16_256_k3", 2, 40, (16, 256), (3,), False, "narrow"),
        _case("narrow_1024_80_k1", 2, 40, (1024, 80), (1,), False, "narrow"),  # 32 chunks
        _case("narrow_80_160_k3_ww", 2, 130, (80, 160), (3,), True, "narrow", wide_w=True),
    ]
    for base in ("narrow_80_80_k1", "narrow_80_160_k3"):
        c = next(c for c in out if c.name == base)
        for ft in (8, 4, 2):
            out.append(c._replace(name=f"{base}_ft{ft}", opts=(("conv_narrow_ft", ft),)))
        out.append(c._replace(name=f"{base}_split", opts=(("conv_split_always", 1),)))     # reading a split image
    # the group-ring form
    ring = _case("ring_128_512_33", 2, 77, (128, 512, 33), (3, 1), form="ring")
    out += [ring, ring._replace(name="ring_128_512_33_noring", opts=(("conv_no_ring", 1),))]
    # fused trailing layers, one per instantiated key
    for key, chans, ks in ((110, (48, 80, 80), (5, 1)), (111, (96, 80, 80, 80), (1, 1, 1)), (210, (64, 160, 80), (1, 1)),
                           (211, (80, 160, 80, 80), (3, 1, 1)), (220, (64, 160, 160), (3, 1))):
        for T in (70, 130):
            # (64 -> 160 -> 160 is the shape the 220 instantiation was written for, but conv_form() gives its 160 -> 160
            # layer the wide form, and fused_plan() asks for narrow layers throughout: a narrow kernel, then a wide one)
            c = _case(f"fused{key}_T{T}", 2, T, chans, ks, form="chain" if key == 220 else f"fused{key}")
            out += [c, c._replace(name=c.name + "_nofuse", opts=(("conv_no_fuse", 1),))]
            if key == 211 and T == 130:
                out.append(c._replace(name=c.name + "_ft8", opts=(("conv_narrow_ft", 8),)))
    # mixed stacks
    out.append(_case("mixed_k5331", 2, 150, (40, 64, 48, 130, 20), (5, 3, 3, 1), form="chain"))   # fp32 temporaries between layers
    out.append(_case("mixed_wide_ring_fused", 2, 150, (128, 512, 64, 64, 64, 48), (3, 1, 1, 1, 1), form="fused111"))
    return out


CASES = {c.name: c for c in _cases()}
CASE_NAMES = tuple(CASES)
BASES = tuple(sorted({c.base for c in CASES.values()}))


def case_layers(c):
    """[(Cin, Cout, K)] of a case."""
    return list(zip(c.chans[:-1], c.chans[1:], c.ks))


# ---- the dispatch's channel rules, restated (conv_form / conv_plan's FT of the wide form / fused_plan): only what
# depends on (Cin, Cout, K, T), nothing that depends on the CU count or the LDS size ----
def conv_form(Cin, Cout, K):
    if Cout >= 128 and Cin >= 128:
        return "wide"
    if Cout <= 256 and Cin >= 16:
        return "narrow"
    return "none"


def wide_ft(T):
    if T > 208:
        return 8 if (T + 127) // 128 * 128 < (T + 207) // 208 * 208 else 13
    return 8 if T <= 128 else 13


def fused_key(layers):
    """The key N0 N1 N2 of the trailing layers conv_narrow_fused_kernel takes (0: none)."""
    cpad = lambda co: (co + 31) // 32 * 32  # noqa: E731
    for cnt in (3, 2):
        if cnt > len(layers):
            continue
        G = layers[len(layers) - cnt:]
        if conv_form(*G[0]) != "narrow" or any(k != 1 or conv_form(ci, co, 1) != "narrow" for ci, co, k in G[1:]):
            continue
        N = [2 if cpad(G[0][1]) > 128 else 1, 0, 0]
        nw = cpad(G[0][1]) // (16 * N[0])
        if nw > 6:
            continue
        ok = True
        for j in range(1, cnt):
            ci, co, _ = G[j]
            N[j] = -(-((co + 15) // 16) // nw)
            ok = ok and N[j] <= 2 and N[j] * nw * 16 <= cpad(co) and N[j - 1] * nw * 16 <= 32 * ((ci + 31) // 32)
        key = 100 * N[0] + 10 * N[1] + N[2]
        if ok and key in (110, 111, 210, 211, 220):
            return key
    return 0


def takes_ring(layers):
    """A k = 1 layer behind a producer (it reads a split image) with 16 or more input chunks, a multiple of four, and
    at most eight waves: conv_narrow_ring_kernel (at the two-tile workgroups small batches get)."""
    for n, (ci, co, k) in enumerate(layers):
        nch, cp = (ci + 31) // 32, (co + 31) // 32 * 32
        if n > 0 and k == 1 and conv_form(ci, co, k) == "narrow" and nch >= 16 and nch % 4 == 0 and cp // (16 * (2 if cp > 128 else 1)) <= 8:
            return True
    return False


def expected_form(c):
    layers = case_layers(c)
    if len(layers) == 1:
        f = conv_form(*layers[0])
        return f + str(wide_ft(c.T)) if f == "wide" else f
    key = fused_key(layers)
    if key:
        return f"fused{key}"
    return "ring" if takes_ring(layers) else "chain"


# ---- one reference per (base case, family): inputs, float64 activations, bounds.  Cached and shared: never modified ----
def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode())


@functools.lru_cache(maxsize=None)
def inputs(base, family):
    """(x fp32 [B,Cin,T], [(w, b or None, relu)]) of a base case.  The `impulse` family runs its first layer without a
    bias: its cells outside every impulse's reach are then exact zeros (E = 0)."""
    c = CASES[base]
    rng = np.random.default_rng(_seed(base, family))
    x = draw(family, rng, (c.B, c.chans[0], c.T))
    layers = []
    L = case_layers(c)
    for n, (ci, co, k) in enumerate(L):
        w, b = draw_weights(rng, co, ci, k, c.wide_w)
        relu = c.relu if len(L) == 1 else n + 1 < len(L)
        layers.append((w, None if (family == "impulse" and n == 0) else b, relu))
    return x, layers


@functools.lru_cache(maxsize=None)
def reference(base, family):
    """(x, layers, want [B,Cout,T] float64, E [B,Cout,T]) of a base case: the last layer's output and its bound."""
    x, layers = inputs(base, family)
    hs, Es = stack_bound(x, layers)
    return x, layers, hs[-1], Es[-1]


def ratio(got, want, E):
    """Largest |got - want| / E over all cells; a cell with E == 0 must be exactly 0 (inf otherwise)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(E > 0, err / E, np.where(np.asarray(got) == 0, 0.0, np.inf))
    return float(r.max())
