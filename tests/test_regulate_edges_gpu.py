"""The mechanisms of the length regulator (aligner_regulate_f32, csrc/prior.hip: regulate_kernel) that
test_hard_objective_gpu.py does not reach: the channel slices of the grid's z axis at the widths of real text encoders
(8 and 16 slices, a short last slice, the 8-wide body with and without a tail), the durations' scan at up to 59 tokens
per thread and its limit, and the calls that ask for only one of the two outputs.  The kernel only copies, so every
comparison is bit for bit, against a numpy gather; the outputs are carved out of NaN-filled allocations and the C ABI
is called on the interior pointers, so an element written by no slice, or a store outside, is visible."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAND = 1024                                      # elements of canary on either side


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def slices(B, C, Ty):
    """The host's choice of channel slices, restated."""
    wgs, nz = -(-Ty // 256) * B, 1
    while nz < 16 and wgs * nz < 2048 and C // (nz * 2) >= 16:
        nz *= 2
    return nz


def reference(h, dur, Ty):
    """(out [B,C,Ty], tok [B,Ty]) by np.repeat: negative durations count as 0, frames past the sum are 0 / -1."""
    B, C, Tx = h.shape
    out, tok = np.zeros((B, C, Ty), np.float32), np.full((B, Ty), -1, np.int32)
    for b in range(B):
        idx = np.repeat(np.arange(Tx), np.maximum(dur[b], 0))[:Ty]
        tok[b, :len(idx)] = idx
        out[b, :, :len(idx)] = h[b][:, idx]
    return out, tok


def channel_tagged(B, C, Tx):
    """h[b,c,x] = 1024 c + x + b / 4: exact in fp32 and different in every element, so a channel written by the wrong
    slice shows."""
    assert Tx <= 1024 and C * 1024 < 2 ** 21
    b, c, x = np.meshgrid(np.arange(B), np.arange(C), np.arange(Tx), indexing="ij")
    return (1024.0 * c + x + 0.25 * b).astype(np.float32)


def three_kinds(Tx, Ty, seed):
    """[3, Tx] durations: zeros and negatives with the sum exactly Ty | a sum short of Ty | a sum past Ty."""
    rng = np.random.default_rng(seed)
    dur = rng.integers(0, 2 * Ty // Tx + 3, (3, Tx)).astype(np.int32)
    dur[:, rng.integers(0, Tx, 6)] = 0
    dur[0, [2, Tx // 2, Tx - 2]] = (-1, -7, -2)
    for b in (0, 1):
        while np.maximum(dur[b], 0).sum() > Ty - 60:
            dur[b, np.argmax(dur[b])] //= 2
    dur[0, -1] = max(dur[0, -1], 0)
    dur[0, -1] += Ty - np.maximum(dur[0], 0).sum()
    assert dur[0, -1] > 0 and np.maximum(dur[0], 0).sum() == Ty
    dur[2, Tx // 3] += max(0, Ty + 50 - np.maximum(dur[2], 0).sum())
    assert np.maximum(dur[1], 0).sum() < Ty < np.maximum(dur[2], 0).sum()
    return dur


def fenced(count, dev):
    buf = torch.full((BAND + count + BAND,), float("nan"), dtype=torch.float32, device=dev)
    return buf, buf[BAND:BAND + count]


def intact(buf, count):
    return bool(torch.isnan(buf[:BAND]).all()) and bool(torch.isnan(buf[BAND + count:]).all())


NAN_BITS = 0x7FC00000                            # torch.full's NaN, seen through an int32 view


def regulate_abi(dev, h, dur, Ty, want_out=True, want_tok=True):
    """aligner_regulate_f32 into NaN-fenced, NaN-filled buffers: (rc, out or None, tok or None) as numpy arrays, after
    asserting that the canaries are intact."""
    from aligner_amd import _lib
    B, C, Tx = h.shape
    hd, dd = torch.from_numpy(h).to(dev), torch.from_numpy(dur).to(dev)
    obuf, o = fenced(B * C * Ty, dev)
    tbuf, t = fenced(B * Ty, dev)
    rc = _lib.load().aligner_regulate_f32(hd.data_ptr() if want_out else None, dd.data_ptr(), o.data_ptr() if want_out else None,
                                          t.data_ptr() if want_tok else None, B, C, Tx, Ty,
                                          torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    assert intact(obuf, B * C * Ty) and intact(tbuf, B * Ty), "a store outside the output"
    out, tok = o.view(B, C, Ty).cpu().numpy(), t.view(torch.int32).view(B, Ty).cpu().numpy()
    if not want_out or rc != 0:
        assert np.isnan(out).all(), "out was not asked for"
    if not want_tok or rc != 0:
        assert (tok == NAN_BITS).all(), "tok was not asked for"
    return rc, out if want_out else None, tok if want_tok else None


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("C,nz", [(127, 4), (128, 8), (129, 8), (255, 8), (256, 16), (257, 16), (520, 16)])
def test_channel_slices(dev, C, nz):
    """B = 3, T_mel = 300: six frame blocks, so the slice count is decided by C alone.  Slices are ceil(C / nz) wide --
    16, 17, 32 and 33 channels: the unrolled body alone and with a tail -- and the last one is short."""
    import aligner_amd
    B, Tx, Ty = 3, 37, 300
    assert slices(B, C, Ty) == nz
    h, dur = channel_tagged(B, C, Tx), three_kinds(Tx, Ty, seed=C)
    want_out, want_tok = reference(h, dur, Ty)
    rc, out, tok = regulate_abi(dev, h, dur, Ty)
    cpz = -(-C // nz)
    missing = np.isnan(out).any(axis=(0, 2))
    wrong = (out.view(np.uint32) != want_out.view(np.uint32)).any(axis=(0, 2))
    print(f"C={C}: {nz} slices of {cpz} channels, the last {C - (nz - 1) * cpz}; channels never written: {np.flatnonzero(missing).tolist()}, "
          f"channels with a wrong element: {np.flatnonzero(wrong).tolist()}")
    assert rc == 0 and np.array_equal(tok, want_tok)
    assert not missing.any() and not wrong.any()
    assert (tok[0] >= 0).all() and (tok[1, -60:] == -1).all() and tok[2, -1] < Tx - 1       # full, short, past
    assert not out[1, :, -60:].view(np.uint32).any()                                       # +0.0 bits past the sum
    o2, t2 = aligner_amd.regulate(torch.from_numpy(h).to(dev), torch.from_numpy(dur).to(dev), Ty)
    assert same_bits(o2.cpu().numpy(), want_out) and np.array_equal(t2.cpu().numpy(), want_tok)


def test_sliced_and_unsliced_grids_agree(dev):
    """C = 256 in 16 slices (B = 2, 300 frames) and in one: 2048 utterances of 40 frames are 2048 frame blocks, at which
    the host stops slicing.  The large batch repeats the small one's two utterances; all of them carry the small one's
    first 40 frames."""
    import aligner_amd
    C, Tx = 256, 37
    h, dur = channel_tagged(2, C, Tx), three_kinds(Tx, 300, seed=1)[1:]
    assert slices(2, C, 300) == 16 and slices(2048, C, 40) == 1 and slices(2046, C, 40) == 2
    hd, dd = torch.from_numpy(h).to(dev), torch.from_numpy(dur).to(dev)
    small, tok_small = aligner_amd.regulate(hd, dd, 300)
    want_out, want_tok = reference(h, dur, 300)
    assert same_bits(small.cpu().numpy(), want_out) and np.array_equal(tok_small.cpu().numpy(), want_tok)
    big, tok_big = aligner_amd.regulate(hd.repeat(1024, 1, 1), dd.repeat(1024, 1), 40)
    torch.cuda.synchronize()
    assert big.shape == (2048, C, 40)
    assert torch.equal(big.view(1024, 2, C, 40).view(torch.int32), small[:, :, :40].view(torch.int32).expand(1024, 2, C, 40))
    assert torch.equal(tok_big.view(1024, 2, 40), tok_small[:, :40].expand(1024, 2, 40))


def sparse_durations(Tx, Ty, seed):
    """[2, Tx]: nearly all 0, a few negatives, a handful of long tokens most of which sit at the far end; utterance 0
    stops short of Ty, utterance 1 runs past it."""
    rng = np.random.default_rng(seed)
    dur = np.zeros((2, Tx), np.int32)
    dur[:, rng.integers(0, Tx, 40)] = -3
    for b, total in enumerate((Ty - 90, Ty + 70)):
        owners = np.unique(np.concatenate(([0, Tx // 2 + 1, Tx - 60, Tx - 59, Tx - 2, Tx - 1], rng.integers(Tx - 3000 if Tx > 3000 else 0, Tx, 5))))
        share = rng.multinomial(total - len(owners), np.ones(len(owners)) / len(owners)) + 1
        dur[b, owners] = share
        assert np.maximum(dur[b], 0).sum() == total
    return dur


@pytest.mark.parametrize("Tx,per", [(2049, 9), (15104, 59)])
def test_scan_with_many_tokens_per_thread(dev, Tx, per):
    """The durations' scan at `per` tokens per thread (15104 is the largest text the LDS holds), the owners of the frames
    at high token indices.  h[b,0,x] = x + 1, so the gather shows the owner."""
    assert -(-Tx // 256) == per
    Ty = 600
    dur = sparse_durations(Tx, Ty, seed=Tx)
    h = np.broadcast_to(np.arange(1, Tx + 1, dtype=np.float32), (2, 1, Tx)).copy()
    want_out, want_tok = reference(h, dur, Ty)
    assert want_tok.max() == Tx - 1 and (want_tok[0, -90:] == -1).all()
    rc, out, tok = regulate_abi(dev, h, dur, Ty)
    bad = int((tok != want_tok).sum())
    print(f"Tx={Tx} ({per} tokens per thread): {bad} of {tok.size} frames with a wrong owner; owners up to {tok.max()}")
    assert rc == 0 and bad == 0 and same_bits(out, want_out)


def test_text_past_the_scan_limit_is_edom(dev):
    from aligner_amd import _lib
    Tx, Ty = 15105, 600
    dur = np.zeros((2, Tx), np.int32)
    dur[:, -1] = 5
    h = np.ones((2, 1, Tx), np.float32)
    rc, _, _ = regulate_abi(dev, h, dur, Ty)                     # (asserts both outputs are untouched)
    assert rc == _lib.EDOM
    import aligner_amd
    with pytest.raises(_lib.AlignerError) as e:
        aligner_amd.regulate(torch.from_numpy(h).to(dev), torch.from_numpy(dur).to(dev), Ty)
    assert e.value.code == _lib.EDOM


@pytest.mark.parametrize("C", [129, 257])
def test_tok_only_and_out_only_calls(dev, C):
    """A null out (and h) with tok_out set, and a null tok_out, give the bits of the joint call and leave the other
    buffer alone."""
    B, Tx, Ty = 3, 37, 300
    h, dur = channel_tagged(B, C, Tx), three_kinds(Tx, Ty, seed=C + 1)
    want_out, want_tok = reference(h, dur, Ty)
    rc, out, tok = regulate_abi(dev, h, dur, Ty)
    assert rc == 0 and same_bits(out, want_out) and np.array_equal(tok, want_tok)
    rc, none, tok1 = regulate_abi(dev, h, dur, Ty, want_out=False)
    assert rc == 0 and none is None and np.array_equal(tok1, tok)
    rc, out1, none = regulate_abi(dev, h, dur, Ty, want_tok=False)
    assert rc == 0 and none is None and same_bits(out1, out)
