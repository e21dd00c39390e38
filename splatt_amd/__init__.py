"""splatt_amd — an MI355X-native sparse tensor factorization engine.

A from-scratch rebuild of the capabilities of SPLATT (the Surprisingly
ParalleL spArse Tensor Toolkit): CPD via ALS around a fast CSF MTTKRP —
designed CDNA4-first: hand-written gfx950 HIP kernels for the sparse hot
path, rocBLAS (through PyTorch-ROCm) for the dense normal equations, RCCL
over xGMI (torch.distributed) for multi-GPU decompositions.
"""

__version__ = "0.1.0"
VERSION = (0, 1, 0)

from splatt_amd.sptensor import SpTensor
from splatt_amd.csf import Csf, CsfSet, CsfAllocPolicy, build_csf, csf_alloc, order_modes
from splatt_amd.mttkrp import (mttkrp, mttkrp_stream, strip_pace_stats,
                               strip_pace_waits)
from splatt_amd.cpd import CpdOptions, Kruskal, cpd_als, cpd_als_cpu_native, seeded_init
from splatt_amd.kruskal import (kruskal_fit, kruskal_innerprod, kruskal_norm,
                                kruskal_to_dense)
from splatt_amd.completion import (CompleteOptions, Completion, complete_als,
                                   complete_update, kruskal_predict, rmse)
from splatt_amd.admm import (AoAdmmOptions, Constraint, ConstrainedKruskal,
                             admm_solve, admm_update, box, cpd_aoadmm, l1,
                             nonneg, nonneg_l1)
from splatt_amd.tucker import Tucker, TuckerOptions, ttmc, tucker_hooi
from splatt_amd.apr import (AprOptions, PoissonKruskal, apr_update,
                            apr_update_pdnr, cpd_apr)
from splatt_amd.gcp import (GcpKruskal, GcpOptions, cpd_gcp, gcp_fg, gcp_grad,
                            sample_zeros)
from splatt_amd.sgcp import (GcpSample, SgcpKruskal, SgcpOptions, adam_step,
                             cpd_sgcp, gcp_sample, gcp_sgrad)

load = SpTensor.load

__all__ = [
    "SpTensor", "Csf", "CsfSet", "CsfAllocPolicy", "build_csf", "csf_alloc",
    "order_modes", "mttkrp", "mttkrp_stream", "strip_pace_stats",
    "strip_pace_waits",
    "CpdOptions", "Kruskal",
    "cpd_als", "cpd_als_cpu_native", "seeded_init", "load",
    "kruskal_fit", "kruskal_innerprod", "kruskal_norm", "kruskal_to_dense",
    "CompleteOptions", "Completion", "complete_als", "complete_update",
    "kruskal_predict", "rmse",
    "AoAdmmOptions", "Constraint", "ConstrainedKruskal", "admm_solve",
    "admm_update", "cpd_aoadmm", "nonneg", "l1", "nonneg_l1", "box",
    "Tucker", "TuckerOptions", "ttmc", "tucker_hooi",
    "AprOptions", "PoissonKruskal", "apr_update", "apr_update_pdnr",
    "cpd_apr",
    "GcpOptions", "GcpKruskal", "gcp_grad", "gcp_fg", "cpd_gcp",
    "sample_zeros",
    "GcpSample", "SgcpOptions", "SgcpKruskal", "gcp_sample", "gcp_sgrad",
    "adam_step", "cpd_sgcp",
]
