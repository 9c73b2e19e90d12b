"""The alignment search's argument checks without a GPU: every refusal of forward_impl and of the entry points around it
that comes before the first HIP call, held to its code and to a piece of its message.  ctypes only, host pointers, no launch.

Not here: aligner_maxpath_scatter_path's unsupported path dtype (it asks for the device's LDS limit first;
tools/maxpath_launches.py lists it on the GPU), and a row pitch together with a mask (aligner_maxpath_ld, the only entry
point with a pitch, takes no mask argument)."""
import numpy as np
import pytest

from aligner_amd import _lib

F32, BF16, F64, I32 = _lib.DT_F32, _lib.DT_BF16, _lib.DT_F64, _lib.DT_I32
NO_SUCH_DTYPE = 99
BUF = np.zeros(1024, np.float32)
P = BUF.ctypes.data


def _forward(lib, value=P, value_dtype=F32, mask=None, mask_dtype=0, t_xs=P, t_ys=P, ws=P, nws=1 << 30, B=1, Tx=4, Ty=8, flags=0):
    return lib.aligner_maxpath_forward(value, value_dtype, mask, mask_dtype, t_xs, t_ys, None, None, ws, nws, B, Tx, Ty, -1e9, flags, None)


def _maxpath(lib, path=P, path_dtype=I32, value_dtype=F32, flags=0, nws=1 << 30):
    return lib.aligner_maxpath(P, value_dtype, None, 0, P, P, path, path_dtype, None, None, P, nws, 1, 4, 8, -1e9, flags, None)


def _maxpath_ld(lib, ld=16, path=None, path_dtype=I32, t_xs=P, Tx=4, Ty=8, flags=0):
    return lib.aligner_maxpath_ld(P, F32, ld, t_xs, P, path, path_dtype, None, None, P, 1 << 30, 1, Tx, Ty, -1e9, flags, None)


REFUSALS = {
    "value null": (lambda lib: _forward(lib, value=None), _lib.EINVAL, b"value/workspace pointer is null"),
    "workspace null": (lambda lib: _forward(lib, ws=None), _lib.EINVAL, b"value/workspace pointer is null"),
    "bad shape": (lambda lib: _forward(lib, Tx=0), _lib.EINVAL, b"bad shape B=1 Tx=0 Ty=8"),
    "Tx*Ty": (lambda lib: _forward(lib, Tx=1 << 16, Ty=1 << 15), _lib.EDOM, b"Tx*Ty=2147483648 exceeds 2^31"),
    "no lengths, no mask": (lambda lib: _forward(lib, t_xs=None), _lib.EINVAL, b"need either lengths (t_xs,t_ys) or a mask"),
    "strict without mask": (lambda lib: _forward(lib, flags=_lib.F_STRICT_MASK), _lib.EINVAL, b"ALIGNER_F_STRICT_MASK needs a mask"),
    "score dtype": (lambda lib: _forward(lib, value_dtype=F64), _lib.EINVAL, b"value dtype 3 not supported (F32, BF16, F16)"),
    "strict mask dtype": (lambda lib: _forward(lib, mask=P, mask_dtype=BF16, flags=_lib.F_STRICT_MASK), _lib.EINVAL,
                          b"strict mask must have the scores' dtype (mask 2, value 0)"),
    "pitch < Ty": (lambda lib: _maxpath_ld(lib, ld=4), _lib.EINVAL, b"ld_value=4 < Ty=8"),
    "pitch with WRITE_Q": (lambda lib: _maxpath_ld(lib, flags=_lib.F_WRITE_Q), _lib.EINVAL,
                           b"a row pitch of its own (ld_value=16, Ty=8) takes lengths, no mask and no ALIGNER_F_WRITE_Q"),
    "Tx*ld": (lambda lib: _maxpath_ld(lib, ld=1 << 29), _lib.EDOM, b"Tx*ld_value=2147483648 exceeds 2^31"),
    "workspace too small": (lambda lib: _forward(lib, nws=lib.aligner_maxpath_workspace_bytes(1, 4, 8) - 1), _lib.ENOSPC, b"workspace "),
    "WRITE_Q on bf16": (lambda lib: _forward(lib, value_dtype=BF16, flags=_lib.F_WRITE_Q), _lib.EINVAL,
                        b"ALIGNER_F_WRITE_Q takes fp32 scores without a strict mask"),
    "ld with strict": (lambda lib: _maxpath_ld(lib, flags=_lib.F_STRICT_MASK), _lib.EINVAL, b"aligner_maxpath_ld takes no mask"),
    "path dtype, maxpath": (lambda lib: _maxpath(lib, path_dtype=NO_SUCH_DTYPE), _lib.EINVAL, b"path dtype 99 not supported"),
    "path dtype, maxpath_ld": (lambda lib: _maxpath_ld(lib, path=P, path_dtype=NO_SUCH_DTYPE), _lib.EINVAL, b"path dtype 99 not supported"),
    "path dtype, zero_path": (lambda lib: lib.aligner_maxpath_zero_path(P, NO_SUCH_DTYPE, 1, 4, 8, 0, None), _lib.EINVAL,
                              b"path dtype 99 not supported"),
    "path dtype, expand_ex": (lambda lib: lib.aligner_maxpath_expand_ex(P, P, NO_SUCH_DTYPE, 1, 4, 8, 0, None), _lib.EINVAL,
                              b"path dtype 99 not supported"),
    "expand_ex, ws null": (lambda lib: lib.aligner_maxpath_expand_ex(None, P, I32, 1, 4, 8, 0, None), _lib.EINVAL, b"null pointer"),
    "expand_ex, path null": (lambda lib: lib.aligner_maxpath_expand_ex(P, None, I32, 1, 4, 8, 0, None), _lib.EINVAL, b"null pointer"),
    "expand_ex, bad shape": (lambda lib: lib.aligner_maxpath_expand_ex(P, P, I32, 1, 4, 0, 0, None), _lib.EINVAL, b"bad shape B=1 Tx=4 Ty=0"),
    "zero_path, path null": (lambda lib: lib.aligner_maxpath_zero_path(None, I32, 1, 4, 8, 0, None), _lib.EINVAL, b"null pointer"),
    "zero_path, bad shape": (lambda lib: lib.aligner_maxpath_zero_path(P, I32, -1, 4, 8, 0, None), _lib.EINVAL, b"bad shape B=-1 Tx=4 Ty=8"),
    "scatter_path, ws null": (lambda lib: lib.aligner_maxpath_scatter_path(None, P, I32, 1, 4, 8, None), _lib.EINVAL, b"null pointer"),
    "scatter_path, path null": (lambda lib: lib.aligner_maxpath_scatter_path(P, None, I32, 1, 4, 8, None), _lib.EINVAL, b"null pointer"),
    "scatter_path, bad shape": (lambda lib: lib.aligner_maxpath_scatter_path(P, P, I32, 1, 0, 8, None), _lib.EINVAL, b"bad shape B=1 Tx=0 Ty=8"),
    "lengths, mask null": (lambda lib: lib.aligner_lengths_from_mask(None, F32, 1, 4, 8, P, P, None), _lib.EINVAL, b"null pointer"),
    "lengths, t_xs null": (lambda lib: lib.aligner_lengths_from_mask(P, F32, 1, 4, 8, None, P, None), _lib.EINVAL, b"null pointer"),
    "lengths, t_ys null": (lambda lib: lib.aligner_lengths_from_mask(P, F32, 1, 4, 8, P, None, None), _lib.EINVAL, b"null pointer"),
    "lengths, bad shape": (lambda lib: lib.aligner_lengths_from_mask(P, F32, 1, 4, 0, P, P, None), _lib.EINVAL, b"bad shape B=1 Tx=4 Ty=0"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusal_before_any_hip_call(built_lib, name):
    call, code, message = REFUSALS[name]
    assert call(built_lib) == code
    assert message in built_lib.aligner_last_error(), built_lib.aligner_last_error()


def test_empty_batch_is_accepted_before_the_workspace_is_looked_at(built_lib):
    assert _forward(built_lib, B=0, nws=0) == 0
    assert built_lib.aligner_maxpath_zero_path(P, I32, 0, 4, 8, 0, None) == 0
    assert built_lib.aligner_maxpath_expand_ex(P, P, I32, 0, 4, 8, 0, None) == 0
    assert built_lib.aligner_lengths_from_mask(P, F32, 0, 4, 8, P, P, None) == 0
