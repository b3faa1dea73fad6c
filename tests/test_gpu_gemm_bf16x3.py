"""pk_gemm(prec = PK_PREC_BF16X3), element by element against float64 with the derived bound of DESIGN.md 4.9,
|C - C64| <= (2^-16 + (K + 8) 2^-24) (|alpha| |A| |B|) + 2^-22 (|beta C_in| + |bias|), and exactly on integer operands."""
import importlib

import pytest
import torch

pytestmark = pytest.mark.gpu
F_ = importlib.import_module("pytorch-kaldi_amd.functional")
LAYOUTS = [(1, 1), (1, 0), (0, 1), (0, 0)]  # (A contiguous along k?, B contiguous along k?)


def _place(logical, k_contig_is_cols, pad, shift):
    """logical [rows, k] -> (device view contiguous along k or along rows, row stride, k stride); ld + pad, base + shift"""
    src = logical if k_contig_is_cols else logical.t()
    r, c = src.shape
    buf = torch.zeros(r * (c + pad) + shift, device="cuda")
    view = buf[shift:].view(r, c + pad)[:, :c]
    view.copy_(src)
    return (view, c + pad, 1) if k_contig_is_cols else (view, 1, c + pad)


def _gemm(A, B, a_kc, b_kc, alpha=1.0, beta=0.0, bias=None, Cin=None, splitk=1, pad=0, shift=0):
    """A [M, K], B [K, N] (CPU fp32) -> C of pk_gemm(prec = 2) on the four storage layouts."""
    (M, K), N = A.shape, B.shape[1]
    Av, a_rs, a_cs = _place(A, a_kc, pad, shift)
    Bv, b_cs, b_rs = _place(B.t(), b_kc, pad, shift)  # rows of the placed matrix are n
    C = (torch.zeros(M, N) if Cin is None else Cin.clone()).cuda()
    F_.gemm(M, N, K, Av, a_rs, a_cs, Bv, b_rs, b_cs, C, N, alpha=alpha, beta=beta,
            bias=None if bias is None else bias.cuda(), splitk=splitk, prec="bf16x3")
    torch.cuda.synchronize()
    return C.cpu()


def _bound(A, B, alpha=1.0, beta=0.0, bias=None, Cin=None):
    """(float64 result, element-wise tolerance) of the derived bound."""
    K = A.shape[1]
    A64, B64 = A.double(), B.double()
    rest = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float64)
    if Cin is not None:
        rest = rest + beta * Cin.double()
    absrest = rest.abs()
    if bias is not None:
        rest, absrest = rest + bias.double(), absrest + bias.double().abs()
    tol = (2.0 ** -16 + (K + 8) * 2.0 ** -24) * abs(alpha) * (A64.abs() @ B64.abs()) + 2.0 ** -22 * absrest
    return alpha * (A64 @ B64) + rest, tol


def _operands(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g) * torch.exp2(torch.randint(-6, 6, s, generator=g).float())  # noqa: E731
    return mk(M, K), mk(K, N), g


VARIANTS = {
    "plain": {},
    "unaligned": {"pad": 3, "shift": 1},  # base off by one float, padded leading dimension: scalar loads
    "splitk3": {"splitk": 3},
    "epilogue": {"alpha": 0.5, "beta": 1.0, "bias": True},
}
CASES = [(s, "plain") for s in ((130, 70, 45), (33, 257, 200), (128, 128, 32), (1, 5, 3))] + [
    ((130, 70, 45), "unaligned"), ((33, 257, 200), "splitk3"), ((130, 70, 45), "epilogue"), ((130, 70, 0), "epilogue")]


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("shape,variant", CASES)
def test_bound_against_float64(shape, variant, a_kc, b_kc):
    M, N, K = shape
    A, B, g = _operands(M, N, K, 1000 + M + K)
    kw = dict(VARIANTS[variant])
    if kw.pop("bias", False):
        kw["bias"], kw["Cin"] = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    C = _gemm(A, B, a_kc, b_kc, **kw)
    ref, tol = _bound(A, B, **{k: v for k, v in kw.items() if k in ("alpha", "beta", "bias", "Cin")})
    assert bool(((C.double() - ref).abs() <= tol).all())


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
@pytest.mark.parametrize("wide_is_a", [True, False])
@pytest.mark.parametrize("M,N,K", [(130, 70, 32), (40, 130, 19)])
def test_exact_on_integers(M, N, K, wide_is_a, a_kc, b_kc):
    """12-bit integers are exactly hi + lo, 7-bit ones exactly bf16, every sum is below 2^24: the product is exact."""
    g = torch.Generator().manual_seed(7 * M + K)
    wide = lambda *s: torch.randint(-4095, 4096, s, generator=g).float()  # noqa: E731
    narrow = lambda *s: torch.randint(-127, 128, s, generator=g).float()  # noqa: E731
    A, B = (wide(M, K), narrow(K, N)) if wide_is_a else (narrow(M, K), wide(K, N))
    assert torch.equal(_gemm(A, B, a_kc, b_kc), (A.double() @ B.double()).float())


@pytest.mark.parametrize("a_kc,b_kc", LAYOUTS)
def test_non_finite_values_stay_in_their_rows(a_kc, b_kc):
    A, B, _ = _operands(130, 70, 45, 5)
    A[3, 7], A[100, 40] = float("inf"), float("nan")
    C = _gemm(A, B, a_kc, b_kc)
    hit = torch.zeros(130, dtype=torch.bool)
    hit[[3, 100]] = True
    assert not bool(torch.isfinite(C[hit]).any())
    ref, tol = _bound(A[~hit], B)
    assert bool(((C[~hit].double() - ref).abs() <= tol).all())  # (a NaN fails the comparison)
