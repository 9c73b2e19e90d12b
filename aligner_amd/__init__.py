"""aligner_amd -- MI355X-native TTS alignment hot path (drop-in for xiaozhah/Aligner's
monotonic_align.maximum_path and the soft-attention front end that feeds it).

    from aligner_amd import maximum_path, align, soft_attention
    import aligner_amd; aligner_amd.install_dropin()   # then: from monotonic_align import maximum_path

All compute is in libaligner_amd.so (hand-written HIP for gfx950, C ABI in
include/aligner_amd.h).  Importing this package does not load the library; the
first call does, and raises if it was not built or no GPU is visible.
"""
from __future__ import annotations

import sys

from .maxpath import Alignment, align, maximum_path, maximum_path_c, read_status  # noqa: F401
from .softattn import (AlignmentEncoderParams, alignment_encoder, conv1d, conv1d_backward, soft_attention,  # noqa: F401
                       soft_attention_backward)
from .objective import (alignment_loss, average_by_duration, beta_binomial_prior, binarization_loss, forward_sum,  # noqa: F401
                        forward_sum_loss, regulate, segment_reduce)
from .mobo import BoundarySearch, boundary_search, boundary_search_backward, soft_boundaries  # noqa: F401
from .pausepath import PauseAlignment, align_with_pauses  # noqa: F401
from .ctcalign import CtcAlignment, ctc_forced_align, ctc_token_spans  # noqa: F401
from .gausslogp import gaussian_align, gaussian_forward_sum_loss, gaussian_logp, gaussian_logp_backward  # noqa: F401
from .gaussnll import gaussian_nll, gaussian_nll_loss  # noqa: F401
from .gaussup import gaussian_upsample, gaussian_upsample_at  # noqa: F401
from .softdtw import soft_dtw, soft_dtw_loss  # noqa: F401
from .l1cost import l1_cost, l1_cost_backward, soft_dtw_l1_loss  # noqa: F401
from .banddtw import (band_to_dense, dense_to_band, l1_cost_banded, l1_cost_banded_backward, soft_dtw_banded,  # noqa: F401
                      soft_dtw_banded_loss, soft_dtw_l1_banded_loss)
from .dtwpath import DtwPath, dtw_path, dtw_path_banded, dtw_path_l1, path_to_dense  # noqa: F401
from .l2cost import (dtw_path_l2, l2_cost, l2_cost_backward, l2_cost_banded, l2_cost_banded_backward, mcd_dtw,  # noqa: F401
                     soft_dtw_l2_banded_loss, soft_dtw_l2_loss)
from .pathcost import (PathRuns, dtw_l1_loss, dtw_l2_loss, mcd_dtw_loss, path_cost, path_cost_backward,  # noqa: F401
                       path_runs)

__all__ = ["Alignment", "align", "maximum_path", "maximum_path_c", "read_status",
           "soft_attention", "soft_attention_backward", "conv1d", "conv1d_backward", "alignment_encoder", "AlignmentEncoderParams",
           "forward_sum", "forward_sum_loss", "beta_binomial_prior", "regulate", "segment_reduce", "average_by_duration", "binarization_loss", "alignment_loss",
           "boundary_search", "boundary_search_backward", "soft_boundaries", "BoundarySearch",
           "align_with_pauses", "PauseAlignment", "ctc_forced_align", "ctc_token_spans", "CtcAlignment", "gaussian_logp", "gaussian_logp_backward", "gaussian_forward_sum_loss",
           "gaussian_align", "gaussian_nll", "gaussian_nll_loss",
           "gaussian_upsample", "gaussian_upsample_at", "soft_dtw", "soft_dtw_loss",
           "l1_cost", "l1_cost_backward", "soft_dtw_l1_loss",
           "dense_to_band", "band_to_dense", "soft_dtw_banded", "soft_dtw_banded_loss", "l1_cost_banded",
           "l1_cost_banded_backward", "soft_dtw_l1_banded_loss",
           "dtw_path", "dtw_path_banded", "dtw_path_l1", "path_to_dense", "DtwPath",
           "l2_cost", "l2_cost_backward", "soft_dtw_l2_loss", "l2_cost_banded", "l2_cost_banded_backward",
           "soft_dtw_l2_banded_loss", "dtw_path_l2", "mcd_dtw",
           "path_runs", "PathRuns", "path_cost", "path_cost_backward", "dtw_l1_loss", "dtw_l2_loss", "mcd_dtw_loss",
           "install_dropin"]


def install_dropin() -> None:
    """Register this package's shim as the top-level `monotonic_align` module, so
    `from monotonic_align import maximum_path` and
    `from monotonic_align.monotonic_align.core import maximum_path_c` (the two
    import paths of the reference, __init__.py:3,6) resolve to the HIP path."""
    from . import monotonic_align as shim
    from .monotonic_align import monotonic_align as inner
    from .monotonic_align.monotonic_align import core
    sys.modules["monotonic_align"] = shim
    sys.modules["monotonic_align.monotonic_align"] = inner
    sys.modules["monotonic_align.monotonic_align.core"] = core
