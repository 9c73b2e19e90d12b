"""gaussian_logp() / gaussian_align() on the GPU against the float64 oracle (tests/gausslogp_oracle.py).

The bound: for every cell inside the lengths |got - oracle| <= 2^-14 S, S the magnitude of what the expanded sum adds up
(the oracle returns it).  The split products are documented as ~2^-16 relative per product (include/aligner_amd.h); a
numpy simulation of the three split products in exact accumulation stays below 2^-16 S on these input families
(tests/test_gausslogp_host.py), plain fp32 accumulation adds a few hundredths of that: 2^-14 leaves a factor of four for
accumulation order and exp in fp32.  Every cell outside the lengths is +0.0 exactly.

Shapes sit at the edges of the kernel's structure: channels that are no multiple of the 16-deep MFMA step or of 8 and the
largest count; the 32-row tile, the pair of tiles a wave owns, more pairs than waves and the longest text; the 32-frame
strip, the 64-frame workgroup, T_mel % 4 != 0 and many workgroups; a batch that is a multiple of 8 (the other block map)."""
import functools

import numpy as np
import pytest
import torch

import gausslogp_oracle as GO
from aligner_amd import align, gaussian_align, gaussian_logp, maximum_path, synth
from aligner_amd.softattn import pitched_logp

pytestmark = pytest.mark.gpu

BOUND = 2.0 ** -14


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


# a covering subset of C x T_text x T_mel: every listed size of every axis at least once
EDGE_SHAPES = [(1, 1, 1), (7, 31, 31), (8, 32, 33), (8, 33, 130), (80, 224, 257), (80, 225, 1000), (192, 300, 130),
               (256, 33, 257), (256, 224, 31), (192, 31, 1), (7, 1, 1000), (1, 300, 257), (8, 1024, 33)]


@functools.lru_cache(maxsize=None)
def make_case(B, C, Tx, Ty, lo=0.5, hi=1.5, mid_lengths=False):
    """Inputs of the tests' family with ragged lengths and the oracle's answer.  Cached and shared: never modified.
    B = 3: the first utterance at full size, one with t_x = 1, one with t_x = 0; mid_lengths: the others drawn in between."""
    rng = np.random.default_rng(100000 * C + 1000 * Tx + Ty + int(100 * lo))
    ty = rng.integers(max(1, Ty // 2), Ty + 1, B).astype(np.int32)
    if mid_lengths:
        tx = rng.integers(1, Tx + 1, B).astype(np.int32)
    else:
        tx = np.array([Tx, 1, 0] + [Tx] * (B - 3), np.int32)[:B]
    tx[0], ty[0] = Tx, Ty
    z, m, s = GO.draw_inputs(rng, B, C, Tx, Ty, lo, hi, t_x=tx)
    value, S, valid = GO.gaussian_logp(z, m, s, tx, ty)
    return dict(z=z, mean=m, logstd=s, t_x=tx, t_y=ty, value=value, S=S, valid=valid)


def run(case, dev, **kw):
    t = {k: torch.from_numpy(case[k]).to(dev) for k in ("z", "mean", "logstd", "t_x", "t_y")}
    return gaussian_logp(t["z"], t["mean"], t["logstd"], t["t_x"], t["t_y"], **kw)


def check(case, got, tag):
    got = got.float().cpu().numpy()
    valid = case["valid"]
    assert np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - case["value"])
    ratio = float((err / case["S"])[valid].max()) if valid.any() else 0.0
    print(f"{tag}: max |err| / S = {ratio * 2.0 ** 16:.3f} * 2^-16, max |err| = {float(err[valid].max()) if valid.any() else 0.0:.3e}")
    assert ratio <= BOUND, (tag, ratio / BOUND)
    masked = np.ascontiguousarray(got[~valid])
    assert not masked.view(np.uint32).any(), f"{tag}: a masked cell is not +0.0"
    return ratio


@pytest.mark.parametrize("C,Tx,Ty", EDGE_SHAPES)
def test_values_at_the_structural_edges(dev, C, Tx, Ty):
    case = make_case(3, C, Tx, Ty)
    got = run(case, dev)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, Tx, Ty) and got.is_contiguous() and not got.requires_grad
    check(case, got, f"[3,{C},{Tx},{Ty}]")


@pytest.mark.parametrize("Tx,Ty", [(70, 200), (225, 130), (33, 257)])
def test_small_sigma_family(dev, Tx, Ty):
    """sigma ~ U(0.05, 2): weights up to 400, where the expanded terms cancel hardest."""
    case = make_case(3, 16, Tx, Ty, 0.05, 2.0)
    check(case, run(case, dev), f"small sigma [3,16,{Tx},{Ty}]")


@pytest.mark.parametrize("B,C,Tx,Ty", [(8, 80, 200, 130), (16, 7, 65, 100), (5, 80, 300, 257)])
def test_lengths_in_between_and_both_block_maps(dev, B, C, Tx, Ty):
    """Lengths strictly inside the extents (row tiles past t_x and frame blocks past t_y skip the contraction), in a batch
    that is a multiple of 8 (an utterance's workgroups share an XCD) and in one that is not."""
    case = make_case(B, C, Tx, Ty, mid_lengths=True)
    check(case, run(case, dev), f"[{B},{C},{Tx},{Ty}]")
    # no lengths: the full extent
    full = gaussian_logp(torch.from_numpy(case["z"]).to(dev), torch.from_numpy(case["mean"]).to(dev),
                         torch.from_numpy(case["logstd"]).to(dev)).cpu().numpy()
    value, S, _ = GO.gaussian_logp(case["z"], case["mean"], case["logstd"])
    assert (np.abs(full - value) <= BOUND * S).all()


@pytest.mark.parametrize("C,Tx,Ty", [(80, 225, 257), (7, 33, 31), (192, 64, 130)])
def test_bf16_output_is_the_rounded_fp32_result(dev, C, Tx, Ty):
    case = make_case(3, C, Tx, Ty)
    f32 = run(case, dev)
    b16 = run(case, dev, out_dtype=torch.bfloat16)
    assert b16.dtype == torch.bfloat16 and b16.is_contiguous()
    assert torch.equal(b16.view(torch.int16), f32.to(torch.bfloat16).view(torch.int16))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C,Tx,Ty", [(80, 225, 257), (8, 33, 1000), (7, 1, 31)])
def test_pitched_output_and_out_views(dev, C, Tx, Ty, dtype):
    case = make_case(3, C, Tx, Ty)
    want = run(case, dev, out_dtype=dtype)
    # pitched=True: same bits at a row pitch of whole 128-byte lines
    p = run(case, dev, out_dtype=dtype, pitched=True)
    assert tuple(p.shape) == (3, Tx, Ty) and (p.stride(1) * p.element_size()) % 128 == 0 and torch.equal(p, want)
    # out= a pitched view: the padding columns are never written
    buf = pitched_logp(3, Tx, Ty, dev, dtype)
    ld = buf.stride(1) if Tx > 1 else buf.stride(0)
    whole = torch.as_strided(buf, (3, Tx, ld), (Tx * ld, ld, 1))
    whole.fill_(float("nan"))
    r = run(case, dev, out=buf)
    assert r.data_ptr() == buf.data_ptr() and torch.equal(buf, want)
    assert ld > Ty and torch.isnan(whole[:, :, Ty:]).all()
    # out= a contiguous view at storage offset 0 of a larger buffer: nothing beyond it is written
    big = torch.full((4, Tx, Ty), float("nan"), dtype=dtype, device=dev)
    view = big[:3]
    assert view.storage_offset() == 0 and view.is_contiguous()
    run(case, dev, out=view)
    assert torch.equal(view, want) and torch.isnan(big[3]).all()


def test_determinism_and_side_stream(dev):
    case = make_case(5, 80, 300, 257, mid_lengths=True)
    a = run(case, dev)
    b = run(case, dev)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        c = run(case, dev)
    side.synchronize()
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))


def test_inputs_the_wrapper_has_to_copy_or_cast(dev):
    case = make_case(3, 80, 225, 257)
    want = run(case, dev)
    z = torch.from_numpy(case["z"]).to(dev)
    m, s = torch.from_numpy(case["mean"]).to(dev), torch.from_numpy(case["logstd"]).to(dev)
    tx, ty = torch.from_numpy(case["t_x"]).to(dev), torch.from_numpy(case["t_y"]).to(dev)
    # a z sliced by one element: not contiguous, copied by the wrapper
    wide = torch.zeros((3, 80, 258), device=dev)
    wide[:, :, 1:] = z
    zs = wide[:, :, 1:]
    assert not zs.is_contiguous() and zs.data_ptr() % 16 == 4
    assert torch.equal(gaussian_logp(zs, m, s, tx, ty), want)
    # contiguous operands that start 4 bytes past a 16-byte boundary: read as they are
    def shifted(t):
        flat = torch.zeros(t.numel() + 1, device=dev)
        flat[1:] = t.reshape(-1)
        v = flat[1:].view(t.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v
    assert torch.equal(gaussian_logp(shifted(z), shifted(m), shifted(s), tx, ty), want)
    # float64 inputs and int64 lengths are cast; a tensor that requires grad gives a result that does not
    got = gaussian_logp(z.double(), m.double().requires_grad_(), s, tx.long(), ty.long())
    assert got.dtype == torch.float32 and not got.requires_grad and torch.equal(got, want)


@pytest.mark.parametrize("n", range(len(GO.PLANTED_CASES)))
def test_gaussian_align_finds_the_planted_alignment(dev, n):
    case = GO.planted_case(n)
    t = {k: torch.from_numpy(case[k]).to(dev) for k in ("z", "mean", "logstd", "t_x", "t_y")}
    res = gaussian_align(t["z"], t["mean"], t["logstd"], t["t_x"], t["t_y"], path_dtype=torch.int32)
    assert np.array_equal(res.durations.cpu().numpy(), case["durations"])
    assert np.array_equal(res.path.cpu().numpy(), case["path"])
    # the two-call form on the dense tensor, through the drop-in
    B, Tx, Ty = case["path"].shape
    mask = torch.from_numpy(synth.prefix_mask(case["t_x"], case["t_y"], Tx, Ty)).to(dev)
    logp = gaussian_logp(t["z"], t["mean"], t["logstd"], t["t_x"], t["t_y"])
    dense = maximum_path(logp, mask.to(logp.dtype))
    assert torch.equal(dense.to(torch.int32), res.path)
    # bf16 intermediate: the search reads it as it is and returns a legal alignment of the same lengths
    r16 = gaussian_align(t["z"], t["mean"], t["logstd"], t["t_x"], t["t_y"], logp_dtype=torch.bfloat16, want_path=False)
    d16 = r16.durations.cpu().numpy()
    assert (d16.sum(1) == case["t_y"]).all() and ((d16 > 0).sum(1) == case["t_x"]).all()
    # and align() on gaussian_logp(pitched=True) is the same call
    lp = gaussian_logp(t["z"], t["mean"], t["logstd"], t["t_x"], t["t_y"], pitched=True)
    assert torch.equal(align(lp, t["t_x"], t["t_y"], path_dtype=torch.int32).path, res.path)
