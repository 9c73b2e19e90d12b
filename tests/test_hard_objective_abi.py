"""CPU-side checks of the hard half of the objective (segment reduction, binarization loss and its gradient): the three
entry points are exported, declared and bound; every argument check answers before any HIP call; the Python functions
exist and refuse to run without a GPU.  No compute here (tests/test_hard_objective_gpu.py has it)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("aligner_segment_reduce_f32", "aligner_bin_loss", "aligner_bin_loss_grad_f32")
OK, EINVAL, EDOM = 0, -22, -33
F32, F16, BF16, F64 = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib(built_lib):
    return built_lib


@pytest.fixture(scope="module")
def p():
    """A non-null host address: the checks under test answer before the pointer is ever used."""
    buf = torch.zeros(64, dtype=torch.float32)
    yield buf.data_ptr()
    del buf


def test_symbols_exported_declared_and_bound(lib):
    from aligner_amd import _lib
    with open(os.path.join(ROOT, "include", "aligner_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), f"{name} not exported"
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} not declared in include/aligner_amd.h"
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["aligner_segment_reduce_f32"][1]) == 9
    assert len(_lib.SIGNATURES["aligner_bin_loss"][1]) == 12
    assert len(_lib.SIGNATURES["aligner_bin_loss_grad_f32"][1]) == 13
    assert lib.aligner_abi_version() == 5                       # additive


def test_null_pointers(lib, p):
    for args in [(None, p, p), (p, None, p), (p, p, None)]:
        assert lib.aligner_segment_reduce_f32(*args, 1, 1, 1, 1, 0, None) == EINVAL
        assert b"null" in lib.aligner_last_error()
    for args in [(None, F32, 4, p, None, -27.0, p, p), (p, F32, 4, None, None, -27.0, p, p),
                 (p, F32, 4, p, None, -27.0, None, p), (p, F32, 4, p, None, -27.0, p, None)]:
        assert lib.aligner_bin_loss(*args, 1, 2, 4, None) == EINVAL
        assert b"null" in lib.aligner_last_error()
    for args in [(None, F32, 4, p, None, -27.0, p, p), (p, F32, 4, None, None, -27.0, p, p),
                 (p, F32, 4, p, None, -27.0, None, p), (p, F32, 4, p, None, -27.0, p, None)]:
        for acc in (0, 1):
            assert lib.aligner_bin_loss_grad_f32(*args, acc, 1, 2, 4, None) == EINVAL
            assert b"null" in lib.aligner_last_error()


@pytest.mark.parametrize("shape", [(-1, 1, 1, 1), (1, -1, 1, 1), (1, 1, -1, 1), (1, 1, 1, -1), (1, 1, 0, 1), (1, 1, 1, 0)])
def test_segment_reduce_bad_shapes(lib, p, shape):
    assert lib.aligner_segment_reduce_f32(p, p, p, *shape, 0, None) == EINVAL
    assert lib.aligner_last_error()


@pytest.mark.parametrize("shape", [(-1, 2, 4), (1, -2, 4), (1, 2, -4), (1, 0, 4), (1, 2, 0)])
def test_bin_loss_bad_shapes(lib, p, shape):
    assert lib.aligner_bin_loss(p, F32, 4, p, None, -27.0, p, p, *shape, None) == EINVAL
    assert lib.aligner_bin_loss_grad_f32(p, F32, 4, p, None, -27.0, p, p, 0, *shape, None) == EINVAL
    assert lib.aligner_bin_loss_grad_f32(p, F32, 4, p, None, -27.0, p, p, 1, *shape, None) == EINVAL


@pytest.mark.parametrize("dtype", [F64, 4, 5, 6, -1, 99])
def test_bad_logp_dtype(lib, p, dtype):
    assert lib.aligner_bin_loss(p, dtype, 4, p, None, -27.0, p, p, 1, 2, 4, None) == EINVAL
    assert b"dtype" in lib.aligner_last_error()
    assert lib.aligner_bin_loss_grad_f32(p, dtype, 4, p, None, -27.0, p, p, 0, 1, 2, 4, None) == EINVAL
    assert b"dtype" in lib.aligner_last_error()


def test_row_pitch_below_the_row(lib, p):
    assert lib.aligner_bin_loss(p, F32, 3, p, None, -27.0, p, p, 1, 2, 4, None) == EINVAL
    assert b"ld_logp" in lib.aligner_last_error()
    assert lib.aligner_bin_loss_grad_f32(p, BF16, 3, p, None, -27.0, p, p, 1, 1, 2, 4, None) == EINVAL
    assert b"ld_logp" in lib.aligner_last_error()


def test_oversized_text_axis(lib, p):
    assert lib.aligner_segment_reduce_f32(p, p, p, 1, 1, 1 << 20, 8, 0, None) == EDOM
    assert b"Tx" in lib.aligner_last_error()
    assert lib.aligner_bin_loss(p, F32, 8, p, None, -27.0, p, p, 1, 1 << 20, 8, None) == EDOM
    assert lib.aligner_bin_loss_grad_f32(p, F32, 8, p, None, -27.0, p, p, 0, 1, 1 << 20, 8, None) == EDOM


def test_empty_batch_is_ok(lib, p):
    assert lib.aligner_segment_reduce_f32(p, p, p, 0, 4, 3, 8, 1, None) == OK
    assert lib.aligner_bin_loss(p, F16, 8, p, p, -27.0, p, p, 0, 3, 8, None) == OK
    assert lib.aligner_bin_loss_grad_f32(p, F32, 8, p, p, -27.0, p, p, 0, 0, 3, 8, None) == OK
    assert lib.aligner_bin_loss_grad_f32(p, F32, 8, p, p, -27.0, p, p, 1, 0, 3, 8, None) == OK


def test_python_functions_exist_and_fail_loudly_without_gpu(lib):
    import aligner_amd
    for name in ("segment_reduce", "average_by_duration", "binarization_loss", "alignment_loss", "regulate"):
        assert callable(getattr(aligner_amd, name)) and name in aligner_amd.__all__
    if lib.aligner_device_count() > 0:
        return                                                  # (the GPU suite runs them)
    frames, dur = torch.zeros(1, 2, 5), torch.ones(1, 3, dtype=torch.int32)
    logp, tok, t = torch.zeros(1, 3, 5), torch.zeros(1, 5, dtype=torch.int32), torch.tensor([3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aligner_amd.segment_reduce(frames, dur)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aligner_amd.average_by_duration(frames, dur)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aligner_amd.regulate(torch.zeros(1, 2, 3, requires_grad=True), dur, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aligner_amd.binarization_loss(logp, tok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        aligner_amd.alignment_loss(logp, t, torch.tensor([5]), tok)
