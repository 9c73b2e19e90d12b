"""soft_attention() forward on the GPU against the float64 oracle (tests/softattn_oracle64.py), on input families, lengths,
priors and layouts the fp32-oracle tests (tests/test_softattn_gpu.py) never leave N(0,1) for.

The bound, for every log-prob of a valid row (none is left out):

    |got - want| <= c Scol + 2^-23 |want| + F

Scol[b,j] = the largest magnitude, over the column's valid rows, of what the expanded logit adds up (the oracle returns it):
an error in any row's logit moves the column's log-sum.  c = 2 O.split_bound(C) for the split-product forms -- 2^-16 from 80
channels on: twice what a numpy simulation of the three bf16 products gives in exact accumulation, the factor for the
fp32 accumulation order -- and 4 O.CHAIN_RATIO[C] for the exact-product form (four times the error of an fp32 product chain
over C channels); tests/test_softattn_host.py derives both.  F = O.F_LSE = 6.5e-6: the log-sum-exp in fp32 with the
hardware's exp2 / log2, four times what fp32 torch.log_softmax loses on exact logits (measured there: 1.61e-6).
Rows >= t_x are -inf bit for bit.  soft: |soft - want| <= 2 (c Scol + F), +0.0 in the rows >= t_x, columns sum to 1 within
Tx 2^-22 plus the same term.  Where include/aligner_amd.h keeps the 1e-4 absolute bound (O.PROMISED_1E_4, temperatures up to
the host's sharp rule) that is asserted as well.

Every kernel form a shape admits is forced through the debug options (forms_for()): the row-tile form ("rt"), the strip form
with one row group ("strip"), the row-group form with one, two or four waves per strip ("nopair", "split2", "split4") and
the exact-product form ("exact").  Batches are B = 3 -- one utterance at full size, one with t_x = 1, one with t_x = 0 --
unless said otherwise."""
import contextlib
import functools

import numpy as np
import pytest
import torch

import softattn_oracle64 as O

pytestmark = pytest.mark.gpu

OPTIONS = (b"softattn_exact", b"softattn_no_pair", b"softattn_split", b"softattn_strips")
FORCE = {"rt": {}, "strip": {b"softattn_strips": 1}, "nopair": {b"softattn_no_pair": 1}, "split2": {b"softattn_split": 2},
         "split4": {b"softattn_split": 4}, "exact": {b"softattn_exact": 1}}
SHARP = {"l2": 0.002, "dot": 0.2}                  # above: the host takes the exact-product kernel
NEG_INF_BITS = 0xFF800000


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
def forced(form):
    from aligner_amd import _lib
    lib = _lib.load()
    try:
        for name, value in FORCE[form].items():
            assert lib.aligner_debug_set_option(name, value) == 0
        yield
    finally:
        _reset()


def forms_for(C, Tx, Ty, prior=False, soft=False):
    """The kernel forms aligner_softattn_ld's dispatch admits for a shape (contiguous, 16-byte aligned operands)."""
    ks = (C + 15) // 16
    KS = 5 if ks <= 5 else 8 if ks <= 8 else 16
    G = 7 if KS <= 8 else 4
    if (Tx + 31) // 32 > G:
        return ["exact"] if (prior and soft) else ["nopair", "split2", "split4", "exact"]
    rt = KS <= 8 and C == 16 * KS and Ty % 4 == 0 and not prior and not soft
    return (["rt"] if rt else []) + ["strip", "exact"]


def lengths3(Tx):
    return (Tx, 1, 0)


@functools.lru_cache(maxsize=None)
def make_case(family, C, Tx, Ty, sim, T, t_x=None, prior=None, seed=0):
    """Inputs of one family and the oracle's answer.  Cached and shared: never modified.  t_x: a tuple (default lengths3)."""
    t_x = np.array(lengths3(Tx) if t_x is None else t_x, np.int32)
    B = len(t_x)
    rng = np.random.default_rng(100000 * C + 1000 * Tx + Ty + 7 * seed + len(family))
    k, q = O.draw(family, rng, B, C, Tx, Ty)
    pr = None
    if prior == "rand0":                                # uniform with 5 % of the cells exactly 0
        pr = rng.random((B, Tx, Ty)).astype(np.float32)
        pr[rng.random((B, Tx, Ty)) < 0.05] = 0.0
    elif prior == "beta":                               # the project's own prior: its far corners underflow to exact zeros
        from aligner_amd import beta_binomial_prior
        full = torch.full((B,), Tx, dtype=torch.int32, device="cuda:0")
        pr = beta_binomial_prior(full, torch.full((B,), Ty, dtype=torch.int32, device="cuda:0"), Tx, Ty).cpu().numpy()
        assert (pr == 0.0).any() and np.isfinite(pr).all() and (pr >= 0).all()
    logp, soft, _, Scol, valid = O.soft_attention(k, q, t_x, pr, T, sim)
    return dict(family=family, C=C, sim=sim, T=T, k=k, q=q, t_x=t_x, prior=pr, logp=logp, soft=soft, Scol=Scol, valid=valid)


def run(case, dev, form, want_soft=False, **kw):
    import aligner_amd
    pr = None if case["prior"] is None else torch.from_numpy(case["prior"]).to(dev)
    k = kw.pop("k", None)
    q = kw.pop("q", None)
    k = torch.from_numpy(case["k"]).to(dev) if k is None else k
    q = torch.from_numpy(case["q"]).to(dev) if q is None else q
    with forced(form):
        out = aligner_amd.soft_attention(k, q, t_x=torch.from_numpy(case["t_x"]).to(dev), prior=pr, temperature=case["T"],
                                         sim=case["sim"], want_soft=want_soft, **kw)
        torch.cuda.synchronize()
    return out


def coeff(form, C):
    return 4 * O.CHAIN_RATIO[C] if form == "exact" else 2 * O.split_bound(C)


def check(case, got, form, soft=None, tag=""):
    """The module docstring's bound on every valid log-prob (and on soft), exact -inf / +0.0 in the masked rows."""
    c = coeff(form, case["C"])
    want, valid, Scol = case["logp"], case["valid"], case["Scol"]
    got = np.ascontiguousarray(got.float().cpu().numpy())
    assert got.shape == want.shape
    assert (got.view(np.uint32)[~valid] == NEG_INF_BITS).all(), f"{tag} {form}: a masked row is not -inf"
    col = c * Scol[:, None, :] + O.F_LSE                 # [B,1,Ty]
    ratio = worst = err_max = 0.0
    if valid.any():
        assert np.isfinite(got[valid]).all(), f"{tag} {form}: a valid log-prob is not finite"
        with np.errstate(invalid="ignore"):
            err = np.where(valid, np.abs(got.astype(np.float64) - want), 0.0)
            bound = np.where(valid, col + 2.0 ** -23 * np.abs(want), np.inf)
        sc = np.broadcast_to(Scol[:, None, :], want.shape)
        ratio = float((err[valid] / sc[valid]).max())
        worst = float((err[valid] / bound[valid]).max())
        err_max = float(err.max())
    print(f"{tag} {case['family']} {case['sim']} T={case['T']:.6g} {form}: max |err| / Scol = {ratio * 2.0 ** 16:.4f} * 2^-16 "
          f"(c = {c * 2.0 ** 16:.4f}), max |err| = {err_max:.3e}, max |err| / bound = {worst:.3f}")
    assert worst <= 1.0, (tag, form, worst)
    promised = (case["sim"], case["family"]) in O.PROMISED_1E_4 and case["T"] <= SHARP[case["sim"]]
    if promised:
        assert err_max < 1e-4, (tag, form, err_max)
    if soft is not None:
        s = np.ascontiguousarray(soft.cpu().numpy())
        assert s.dtype == np.float32 and not np.isnan(s).any(), f"{tag} {form}: NaN in soft"
        assert not s.view(np.uint32)[~valid].any(), f"{tag} {form}: soft is not +0.0 in a masked row"
        serr = np.abs(s.astype(np.float64) - case["soft"])
        sworst = float((serr / (2 * col)).max())
        Tx = want.shape[1]
        sums = s.astype(np.float64).sum(1)               # [B,Ty]
        target = (np.clip(case["t_x"].astype(np.int64), 0, Tx) > 0).astype(np.float64)[:, None]
        sumworst = float((np.abs(sums - target) / (Tx * 2.0 ** -22 + 2 * col[:, 0, :])).max())
        print(f"{tag} {form}: soft max |err| = {float(serr.max()):.3e} ({sworst:.3f} of its bound), column sums {sumworst:.3f} of theirs")
        assert sworst <= 1.0 and sumworst <= 1.0, (tag, form, sworst, sumworst)
    return ratio


def run_and_check(case, dev, form, tag=""):
    """One form on one case: log-probs alone (the plain store paths) and, where the form has a soft output, with it."""
    logp, none = run(case, dev, form)
    assert none is None and logp.dtype == torch.float32 and logp.is_contiguous()
    check(case, logp, form, tag=tag)
    if form != "rt" and not (case["prior"] is not None and form in ("nopair", "split2", "split4")):
        logp2, soft = run(case, dev, form, want_soft=True)
        check(case, logp2, form, soft=soft, tag=tag + " +soft")
    return logp


SHAPES = O.GPU_SHAPES
TEMPS = [("l2", 0.0005), ("l2", 0.002), ("dot", 0.11)]


# ---- 1. families x forms ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family", O.FAMILIES)
@pytest.mark.parametrize("C,Tx,Ty", SHAPES)
def test_families_on_every_form(dev, C, Tx, Ty, family):
    for sim, T in TEMPS:
        case = make_case(family, C, Tx, Ty, sim, T)
        for form in forms_for(C, Tx, Ty):
            run_and_check(case, dev, form, tag=f"[3,{C},{Tx},{Ty}]")


# ---- 2. both sides of the sharp rule ------------------------------------------------------------------------------------

def _next(x):
    return float(np.nextafter(np.float32(x), np.float32(1)))


@pytest.mark.parametrize("family", ["scale3", "planted"])
@pytest.mark.parametrize("C,Tx,Ty", [(80, 200, 132), (80, 225, 130), (256, 129, 96)])
@pytest.mark.parametrize("sim,T,sharp", [("l2", 0.002, False), ("l2", _next(0.002), True), ("dot", 0.2, False),
                                         ("dot", _next(0.2), True), ("l2", 0.05, True)])
def test_both_sides_of_the_sharp_rule(dev, sim, T, sharp, C, Tx, Ty, family):
    """Up to the rule the default call is a split-product form (and every form holds its bound); one fp32 step above it the
    default call is the exact-product kernel, bit for bit.  L2 at 0.05: logits that span hundreds of nats."""
    import aligner_amd
    case = make_case(family, C, Tx, Ty, sim, T)
    tag = f"[3,{C},{Tx},{Ty}]"
    k, q, t = (torch.from_numpy(case[n]).to(dev) for n in ("k", "q", "t_x"))
    default, dsoft = aligner_amd.soft_attention(k, q, t_x=t, temperature=T, sim=sim, want_soft=True)
    exact, esoft = run(case, dev, "exact", want_soft=True)
    same = torch.equal(default.view(torch.int32), exact.view(torch.int32)) and torch.equal(dsoft.view(torch.int32), esoft.view(torch.int32))
    if sharp:
        assert same, "above the rule the default call is not the exact-product kernel"
        check(case, default, "exact", soft=dsoft, tag=tag + " default")
    else:
        assert not same, "at the rule the default call is the exact-product kernel already"
        check(case, default, "strip", soft=dsoft, tag=tag + " default")       # (any split-product form: the same c)
        for form in forms_for(C, Tx, Ty):
            run_and_check(case, dev, form, tag=tag)
    got = default.cpu().numpy()
    assert np.isfinite(got[case["valid"]]).all() and np.isneginf(got[~case["valid"]]).all()
    if T == 0.05 and family == "planted" and C == 256:
        assert (dsoft.cpu().numpy()[case["valid"]] == 0.0).any() and case["logp"][case["valid"]].min() < -200


# ---- 3. text-length edges -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", [0, -3])
@pytest.mark.parametrize("sim,T", [("l2", 0.0005), ("dot", 0.11)])
@pytest.mark.parametrize("C,Tx,Ty", [(80, 225, 130), (80, 64, 132)])
def test_text_length_edges(dev, C, Tx, Ty, sim, T, first):
    """t_x = 0, 1, the 32-row tile edges, Tx - 1, Tx and past Tx (clamped), and a negative one (clamped to 0), in a batch of 8
    (the XCD-aware block map): row tiles wholly masked, a second row group partly or wholly masked.  An utterance with
    t_x <= 0 has log-probs -inf and soft +0.0 throughout -- no NaN (check() asserts both for every masked row)."""
    t_x = (first, 1, 31, 32, 33, Tx - 1, Tx, Tx + 5)
    case = make_case("unit", C, Tx, Ty, sim, T, t_x=t_x)
    assert not case["valid"][0].any() and case["valid"][7].all() and case["valid"][6].all() and not case["valid"][5, Tx - 1].any()
    for form in forms_for(C, Tx, Ty):
        run_and_check(case, dev, form, tag=f"[8,{C},{Tx},{Ty}] t_x[0]={first}")


# ---- 4. priors ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["beta", "rand0"])
@pytest.mark.parametrize("sim,T", [("l2", 0.0005), ("dot", 0.11)])
def test_priors_with_exact_zeros(dev, kind, sim, T):
    """log(prior + 1e-8) with prior = 0 exactly: log(1e-8) -- on the strip and exact forms with the soft output (its second
    normalisation), and on the row-group forms (Tx = 225), which take a prior for the log-probs alone."""
    for (C, Tx, Ty) in [(80, 200, 260), (80, 225, 260)]:
        case = make_case("unit", C, Tx, Ty, sim, T, prior=kind)
        assert (case["prior"] == 0.0).any()
        forms = forms_for(C, Tx, Ty, prior=True)
        assert forms == (["strip", "exact"] if Tx == 200 else ["nopair", "split2", "split4", "exact"])
        for form in forms:
            run_and_check(case, dev, form, tag=f"[3,{C},{Tx},{Ty}] prior {kind}")


@pytest.mark.parametrize("C,Tx", [(80, 225), (256, 129)])
def test_soft_with_a_prior_beyond_one_row_group_is_refused(dev, C, Tx):
    import aligner_amd
    from aligner_amd._lib import EDOM, AlignerError
    k, q = torch.zeros(1, C, Tx, device=dev), torch.zeros(1, C, 8, device=dev)
    prior = torch.ones(1, Tx, 8, device=dev)
    with pytest.raises(AlignerError, match=f"soft output with a prior needs Tx <= {224 if C == 80 else 128}") as e:
        aligner_amd.soft_attention(k, q, prior=prior, want_soft=True)
    assert e.value.code == EDOM
    aligner_amd.soft_attention(k, q, prior=prior)                         # the log-probs alone are served


# ---- 5. bf16 output -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,Tx,Ty", [(80, 200, 132), (80, 225, 130), (256, 129, 96), (7, 31, 1)])
def test_bf16_log_probs_are_the_fp32_ones_rounded(dev, C, Tx, Ty):
    for sim, T in (("l2", 0.0005), ("dot", 0.11)):
        case = make_case("scale3", C, Tx, Ty, sim, T)
        for form in forms_for(C, Tx, Ty):
            f32, _ = run(case, dev, form)
            b16, _ = run(case, dev, form, logp_dtype=torch.bfloat16)
            assert b16.dtype == torch.bfloat16
            assert torch.equal(b16.view(torch.int16), f32.bfloat16().view(torch.int16)), (form, sim)


# ---- 6. layout ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,Tx,Ty", [(80, 200, 132), (128, 33, 1000)])
def test_row_pitch_gives_the_same_bits(dev, C, Tx, Ty):
    from aligner_amd.softattn import pitched_logp
    case = make_case("scale3", C, Tx, Ty, "l2", 0.0005)
    flat, _ = run(case, dev, "rt")
    check(case, flat, "rt", tag=f"[3,{C},{Tx},{Ty}]")
    own, _ = run(case, dev, "rt", pitched=True)
    assert own.stride(1) % 32 == 0 and own.stride(1) >= Ty and not own.is_contiguous()
    assert torch.equal(own.view(torch.int32), flat.view(torch.int32))
    out = pitched_logp(3, Tx, Ty, dev)
    ld = out.stride(1)
    whole = torch.as_strided(out, (3, Tx, ld), (Tx * ld, ld, 1))
    whole.fill_(float("nan"))
    got, _ = run(case, dev, "rt", out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got.view(torch.int32), flat.view(torch.int32))
    assert ld > Ty and bool(torch.isnan(whole[:, :, Ty:]).all())
    # a sharp temperature: the exact-product kernel has no row pitch, pitched=True falls back to a contiguous tensor
    sharp = make_case("scale3", C, Tx, Ty, "l2", 0.05)
    got, _ = run(sharp, dev, "rt", pitched=True)
    assert got.is_contiguous()
    check(sharp, got, "exact", tag=f"[3,{C},{Tx},{Ty}] pitched, sharp")


@pytest.mark.parametrize("which", ["queries", "keys"])
def test_operand_four_bytes_past_a_16_byte_boundary(dev, which):
    """Contiguous, but not aligned for the row-tile form's 16-byte fetches of the mel operand: the dispatch leaves that form
    for misaligned queries; misaligned keys are read word by word in every form."""
    C, Tx, Ty = 80, 200, 132
    case = make_case("scale3", C, Tx, Ty, "l2", 0.0005)

    def shifted(a):
        buf = torch.empty(a.size + 1, dtype=torch.float32, device=dev)
        t = buf[1:].view(a.shape)
        t.copy_(torch.from_numpy(a))
        assert t.is_contiguous() and t.data_ptr() % 16 == 4
        return t
    kw = {"q": shifted(case["q"])} if which == "queries" else {"k": shifted(case["k"])}
    got, _ = run(case, dev, "rt", **kw)                                    # (nothing forced: the dispatch's own choice)
    check(case, got, "strip", tag=f"[3,{C},{Tx},{Ty}] {which} + 4 bytes")
    ref, _ = run(case, dev, "strip" if which == "queries" else "rt")
    assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    for form in ("strip", "exact"):
        got, soft = run(case, dev, form, want_soft=True, **kw)
        check(case, got, form, soft=soft, tag=f"[3,{C},{Tx},{Ty}] {which} + 4 bytes")


# ---- 7. containment of non-finite inputs --------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("C,Tx,Ty", [(80, 200, 132), (80, 225, 130)])
def test_a_non_finite_query_stays_in_its_column(dev, C, Tx, Ty, bad):
    """One NaN / +inf in queries[b, c, j0]: every other column keeps the clean run's bits, on every form (column j0 itself
    is not asserted)."""
    for sim, T in (("l2", 0.0005), ("dot", 0.11)):
        case = make_case("unit", C, Tx, Ty, sim, T)
        for form in forms_for(C, Tx, Ty):
            soft = form != "rt"
            clean = run(case, dev, form, want_soft=soft)
            for j0 in (0, 35, Ty - 1):
                q = torch.from_numpy(case["q"]).to(dev)
                q[0, 17, j0] = bad
                q[1, C - 1, j0] = bad
                dirty = run(case, dev, form, want_soft=soft, q=q)
                keep = torch.ones(Ty, dtype=torch.bool, device=dev)
                keep[j0] = False
                for a, b in zip(clean, dirty):
                    if a is not None:
                        assert torch.equal(a[:, :, keep].view(torch.int32), b[:, :, keep].view(torch.int32)), (form, sim, j0)


# ---- 8. determinism -----------------------------------------------------------------------------------------------------

def test_every_form_gives_the_same_bits_again(dev):
    C, Tx, Ty = 80, 225, 130
    case = make_case("scale3", C, Tx, Ty, "l2", 0.0005, t_x=(Tx, 1, 100, 224, 193))
    side = torch.cuda.Stream(dev)
    for form in forms_for(C, Tx, Ty):
        a = run(case, dev, form, want_soft=True)
        b = run(case, dev, form, want_soft=True)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            c = run(case, dev, form, want_soft=True)
        for other in (b, c):
            for x, y in zip(a, other):
                assert torch.equal(x.view(torch.int32), y.view(torch.int32)), form
