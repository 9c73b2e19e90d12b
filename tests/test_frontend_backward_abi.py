"""CPU-side checks of the front end's backward entry points (no GPU): exported and in the ctypes table, argument checks
before any device lookup, and every new kernel in the compiler's resource reports with no scratch."""
import glob
import importlib.util
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["aligner_softattn_backward_workspace_bytes", "aligner_softattn_backward_f32", "aligner_conv1d_prepare_transposed_f32",
       "aligner_conv1d_backward_workspace_bytes", "aligner_conv1d_backward_weight_f32"]


def test_backward_symbols_exported_and_declared(built_lib):
    import ctypes

    from aligner_amd import _lib
    with open(os.path.join(ROOT, "include", "aligner_amd.h")) as f:
        header = f.read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW:
        assert n + "(" in header, n
        assert hasattr(raw, n), n
        assert n in _lib.SIGNATURES, n
    assert built_lib.aligner_abi_version() == 5


def test_softattn_backward_argument_checks(built_lib):
    from aligner_amd import _lib
    lib = built_lib
    buf = torch.zeros(64, dtype=torch.float32)
    p = buf.data_ptr()
    B, C, Tx, Ty = 2, 80, 50, 130
    need = lib.aligner_softattn_backward_workspace_bytes(B, C, Tx, Ty)
    assert need >= B * 4 * Ty * 4
    big = 1 << 30

    def call(gk=p, gq=p, ws_bytes=big, C=C, Tx=Tx, sim=_lib.SIM_L2):
        return lib.aligner_softattn_backward_f32(p, p, None, None, p, None, gk, gq, p, ws_bytes, B, C, Tx, Ty, 0.0005, sim,
                                                 None)

    assert call(gk=None, gq=None) == _lib.EINVAL and b"NULL" in lib.aligner_last_error()
    assert call(C=300) == _lib.EDOM and b"256" in lib.aligner_last_error()
    assert call(Tx=600) == _lib.EDOM and b"512" in lib.aligner_last_error()
    assert call(sim=7) == _lib.EINVAL and b"sim" in lib.aligner_last_error()
    assert call(ws_bytes=need - 1) == _lib.ENOSPC


def test_conv_backward_argument_checks(built_lib):
    from aligner_amd import _lib
    lib = built_lib
    buf = torch.zeros(64, dtype=torch.float32)
    p = buf.data_ptr()
    big = 1 << 30
    B, Ci, Co, T = 2, 16, 32, 40
    assert lib.aligner_conv1d_backward_workspace_bytes(B, Ci, Co, T, 3) >= Co * Ci * 3 * 4
    assert lib.aligner_conv1d_backward_workspace_bytes(B, Ci, Co, T, 7) == 0
    rc = lib.aligner_conv1d_backward_weight_f32(p, p, p, p, p, p, p, big, B, Ci, Co, T, 7, 1, None)
    assert rc == _lib.EDOM and b"kernel size" in lib.aligner_last_error()
    rc = lib.aligner_conv1d_backward_weight_f32(p, p, p, None, None, None, p, big, B, Ci, Co, T, 3, 1, None)
    assert rc == _lib.EINVAL
    rc = lib.aligner_conv1d_backward_weight_f32(p, None, p, None, p, p, p, big, B, Ci, Co, T, 3, 1, None)
    assert rc == _lib.EINVAL and b"relu" in lib.aligner_last_error()
    need = lib.aligner_conv1d_backward_workspace_bytes(B, Ci, Co, T, 3)
    rc = lib.aligner_conv1d_backward_weight_f32(p, p, p, None, p, p, p, need - 1, B, Ci, Co, T, 3, 1, None)
    assert rc == _lib.ENOSPC
    rc = lib.aligner_conv1d_prepare_transposed_f32(p, p, big, Co, Ci, 7, None)
    assert rc == _lib.EDOM
    # the transposed image is sized as the forward image of the transposed layer
    assert lib.aligner_conv1d_prepare_transposed_f32(p, p, lib.aligner_conv1d_prepared_bytes(Ci, Co, 3) - 1, Co, Ci, 3,
                                                     None) == _lib.ENOSPC


def test_backward_kernels_have_no_scratch():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = [(name, v) for f in sorted(glob.glob(os.path.join(kr.OBJ, "*.hip.resources.txt"))) for name, v in kr.parse(f)]
    for key in ("softattn_bwd_col_kernel", "softattn_bwd_row_kernel", "conv_bwd_w_kernel", "conv_bwd_reduce_kernel",
                "conv_bwd_mask_kernel"):
        mine = [(n, v) for n, v in rows if key in n]
        assert mine, f"{key} missing from the resource reports"
        for n, v in mine:
            assert not v.get("VGPRs Spill", 0) and not v.get("ScratchSize [bytes/lane]", 0), (n, v)
