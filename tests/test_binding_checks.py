"""Every gpu_* binding validates its tensors before anything is launched.

Runs without a GPU, on purpose: handed correctly shaped HOST tensors, a
binding has to raise RuntimeError naming the argument instead of passing a
host pointer to a kernel. With a device present the same calls would launch,
so the module is skipped there. Without a device every tensor is a host
tensor, so the check that fires is the one on the first tensor a binding
looks at; that tensor is also the one given a wrong dtype.
"""
import pytest
import torch

from splatt_amd._ext import native

pytestmark = pytest.mark.skipif(
    torch.cuda.is_available(),
    reason="host tensors must never reach a device; needs a GPU-less box")

F = 8          # rank
NNZ = 12       # nonzeros
ROWS = 5       # output rows
F64, F32, I32, I64 = (torch.float64, torch.float32, torch.int32, torch.int64)


def vals(dtype=F64):
    return torch.ones(NNZ, dtype=dtype)


def idx(n=2):
    return [torch.zeros(NNZ, dtype=I32) for _ in range(n)]


def mats(n=2, dtype=F64):
    return [torch.ones(4, F, dtype=dtype) for _ in range(n)]


def out(cols=F):
    return torch.zeros(ROWS, cols, dtype=F64)


def blocks():
    return [torch.tensor([0], dtype=I64), torch.tensor([NNZ], dtype=I64),
            torch.tensor([0], dtype=I32)]


def seg_batch():
    """seg_start, seg_len, seg_row, seg_slot, seg0, nseg, mrow, mslot, m0,
    nm, slot0, nslots: one single-segment row."""
    return [torch.tensor([0], dtype=I64), torch.tensor([NNZ], dtype=I32),
            torch.tensor([0], dtype=I32), torch.tensor([-1], dtype=I32), 0, 1,
            torch.zeros(0, dtype=I32), torch.zeros(1, dtype=I64), 0, 0, 0, 0]


def square(dtype=F64):
    return torch.eye(F, dtype=dtype)


def tall(dtype=F64):
    return torch.ones(ROWS, F, dtype=dtype)


def vec(n=F):
    return torch.zeros(n, dtype=F64)


# binding -> (positional arguments without the stream, position and name of
# the first tensor the binding checks)
CASES = {
    "gpu_mttkrp3": lambda: (
        [0, torch.tensor([0, 2], dtype=I64), None,
         torch.tensor([0, 6, NNZ], dtype=I64), torch.zeros(2, dtype=I32),
         torch.zeros(NNZ, dtype=I32), vals(), tall(), tall(), out()],
        1, "fptr0"),
    "gpu_mttkrp_flat": lambda: (
        [torch.zeros(NNZ, dtype=I32), idx(), mats(), vals(), out()],
        3, "vals"),
    "gpu_mttkrp_flat_rp": lambda: (
        [torch.tensor([0, NNZ], dtype=I64), 0, idx(), mats(), vals(), out()],
        4, "vals"),
    "gpu_mttkrp_flat_v32": lambda: (
        [None, 0, torch.zeros(NNZ, dtype=I32), idx(), mats(), vals(F32),
         out()],
        5, "vals"),
    "gpu_mttkrp_flat_det": lambda: (
        [torch.zeros(NNZ, dtype=I32), idx(), mats(), vals(), out(),
         vec(2 * 8 * F)],
        3, "vals"),
    "gpu_mttkrp_flat5": lambda: (
        [torch.zeros(NNZ, dtype=I32), idx(), mats(), vals(), *blocks(), 4, 4,
         out()],
        3, "vals"),
    "gpu_mttkrp_flat6": lambda: (
        [torch.zeros(NNZ, 4, dtype=I32), mats(), vals(), *blocks(), 4, 4,
         out()],
        2, "vals"),
    "gpu_mttkrp_det6": lambda: (
        [torch.zeros(NNZ, 4, dtype=I32), mats(), vals(), *blocks(),
         torch.tensor([0], dtype=I64), 4, 4, 1, vec(ROWS * F),
         vec(4 * 8 * 2 * F), out()],
        2, "vals"),
    "gpu_gram": lambda: ([tall(), square()], 0, "A"),
    "gpu_gram_det": lambda: ([tall(), vec(F * F), square()], 0, "A"),
    "gpu_rowsolve": lambda: ([tall(), square(), tall()], 0, "A"),
    "gpu_spd_inverse": lambda: ([square(), square()], 0, "G"),
    "gpu_colacc": lambda: ([tall(), 0, vec()], 0, "A"),
    "gpu_colscale": lambda: ([tall(), vec()], 0, "A"),
    "gpu_coldot": lambda: ([tall(), tall(), vec()], 0, "X"),
    "gpu_complete_update": lambda: (
        [idx(), mats(), vals(), *seg_batch(), 0.1, vec(1), out()],
        2, "vals"),
    "gpu_kruskal_predict": lambda: (
        [torch.zeros(3, NNZ, dtype=I64), mats(3), None, vec(NNZ)],
        0, "inds"),
    "gpu_ttmc": lambda: (
        [idx(), mats(), vals(), *seg_batch(), vec(1), out(F * F)],
        2, "vals"),
    "gpu_admm_update": lambda: (
        [tall(), square(), vec(1), tall(), tall(), torch.zeros(1, dtype=I32),
         0, 0.0, 0.0, 0.0, 1e-2, 5, 0],
        0, "K"),
    "gpu_als_prep": lambda: (
        [[square(), square()], 0.0, square(), square(), vec(), None],
        2, "Ginv"),
    "gpu_als_tail": lambda: (
        [torch.ones(ROWS, 16, dtype=F64), torch.eye(16, dtype=F64),
         torch.ones(ROWS, 16, dtype=F64), vec(16), torch.eye(16, dtype=F64),
         None],
        0, "K"),
}


def test_every_gpu_binding_is_covered():
    bound = {n for n in dir(native()) if n.startswith("gpu_")}
    assert bound == set(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_tensor_is_rejected(name):
    args, _, first = CASES[name]()
    with pytest.raises(RuntimeError, match=f"{first} must be a device tensor"):
        getattr(native(), name)(*args, 0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_wrong_dtype_is_rejected(name):
    args, pos, first = CASES[name]()
    # no binding takes int16 anywhere, so this is wrong for every argument
    args[pos] = args[pos].to(torch.int16)
    with pytest.raises(RuntimeError, match=f"{first} has dtype Short"):
        getattr(native(), name)(*args, 0)
