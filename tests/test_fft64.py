"""The fp64 mixed-radix Stockham transform fft64 / stage64<R> (sg_fft64_dev.h) alone,
through the hook sg_debug_fft64, at every radix and stage order it accepts, both
directions, against a direct O(M^2) DFT in long double.

The bound is derived, not measured on the kernel:

    TOL64(M) = 4 * 2^-52 * sqrt(sum over the stages of (R_s + 3))

in the relative 2-norm of a frame, the stage radices R_s in fft64's own order. Each
radix-R stage adds R terms and takes one twiddle product; rounding grows as a random
walk over the stages (the square root); 4 is headroom. The CPU tests show that an
fp64 numpy restatement of the same algorithm (the twiddle in place, the direct R-term
sums, correctly rounded roots) stays within TOL64 / 4 of the reference at every size
of the sweep, so the bound is one the algorithm meets before a GPU is asked.

M = 1102 always takes fft64's hand-specialised branch (2 x 19 x 29 with the sizes
folded); the generic loop cannot be sent there from outside, so 1102 is compared with
the reference only."""
import ctypes as C
import functools

import numpy as np
import pytest

LD = np.longdouble
CLD = np.clongdouble
ODD = (3, 5, 7, 11, 13, 17, 19, 23, 29, 31)
RADICES = (2, 4) + ODD

SIZES = sorted(set(
    [2, 3, 4, 5, 7, 11, 13, 17, 19, 23, 29, 31]          # every radix alone
    + [1, 6, 8, 12, 14, 28]                              # the trivial sizes
    + [49, 77, 143, 221, 323, 437, 667, 899, 961, 275, 609, 612, 1001, 1102, 1309, 1426, 1922, 2023, 2025,
       2046, 2048]))


def stages(M):
    """The stage radices of an M-point fft64, in its order: 4s, then a 2, then the odd primes upwards."""
    out, rest = [], M
    while rest > 1:
        R = 4 if rest % 4 == 0 else 2 if rest % 2 == 0 else next(p for p in ODD if rest % p == 0)
        out.append(R)
        rest //= R
    return out


def tol64(M, extra=()):
    return 4 * 2.0 ** -52 * float(np.sqrt(sum(R + 3 for R in list(stages(M)) + list(extra))))


def roots_ld(M):
    """W_M^t = exp(-2 pi i t / M), t < M, in long double; exact at the quadrant points."""
    pi = LD(4) * np.arctan(LD(1))
    ang = (LD(2) * pi) * np.arange(M).astype(LD) / LD(M)
    w = np.cos(ang).astype(CLD) - CLD(1j) * np.sin(ang).astype(CLD)
    for q, v in enumerate((1, -1j, -1, 1j)):
        if (q * M) % 4 == 0:
            w[q * M // 4] = v
    return w


def dft_ld(x, inverse=False):
    """The direct DFT of the rows of x in long double: out[f, j] = sum_k x[f, k] W^(jk mod M),
    the index reduced in integers, the table applied in row blocks of 128."""
    x = np.atleast_2d(x).astype(CLD)
    M = x.shape[1]
    w = roots_ld(M)
    if inverse:
        w = w.conj()
    k = np.arange(M, dtype=np.int64)
    out = np.empty_like(x)
    for j0 in range(0, M, 128):
        j = np.arange(j0, min(M, j0 + 128), dtype=np.int64)
        out[:, j] = x @ w[(j[:, None] * k[None, :]) % M].T
    return out


def rel_err(got, want):
    d = np.asarray(got).astype(CLD) - want
    return float(np.sqrt((np.abs(d) ** 2).sum() / (np.abs(want) ** 2).sum()))


def fft64_numpy(x, inverse=False):
    """fft64 restated in fp64 numpy: Stockham autosort; per stage of radix R every input
    times its twiddle W_{Ns R}^(r (j mod Ns)) in place, then output k of butterfly j is the
    direct sum over m of x_m W_R^(m k), written to (j - j mod Ns) R + j mod Ns + k Ns."""
    a = np.array(x, np.complex128)
    M = a.shape[-1]
    w = roots_ld(M).astype(np.complex128)  # the long-double roots rounded once
    if inverse:
        w = w.conj()
    Ns = 1
    for R in stages(M):
        nR = M // R
        q = np.arange(M)
        a = a * w[(q // nR) * ((q % nR) % Ns) * (M // (Ns * R))]
        j = np.arange(nR)
        base = (j - j % Ns) * R + j % Ns
        xs = a.reshape(a.shape[:-1] + (R, nR))
        b = np.empty_like(a)
        for k in range(R):
            acc = xs[..., 0, :].copy()
            for m in range(1, R):
                acc += xs[..., m, :] * w[((m * k) % R) * nR]
            b[..., base + k * Ns] = acc
        a, Ns = b, Ns * R
    return a


@functools.lru_cache(maxsize=None)
def noise_case(M):
    """Complex Gaussian noise seeded by M and its long-double DFTs (forward, inverse): computed
    once, shared by the CPU and the GPU tests, never written to."""
    rng = np.random.default_rng(M)
    x = rng.normal(size=M) + 1j * rng.normal(size=M)
    want = (dft_ld(x, False)[0], dft_ld(x, True)[0])
    x.setflags(write=False)
    for v in want:
        v.setflags(write=False)
    return x, want


# ---- CPU -------------------------------------------------------------------

def test_long_double_is_wider_than_double():
    assert np.finfo(LD).eps <= 2.0 ** -63


def test_every_radix_first_and_later():
    """Over SIZES every stage64<R> runs as the first stage (Ns = 1, no twiddles) and as a
    later one (twiddles, strided writes), and every odd radix behind 2, 4 and another odd one."""
    first = {stages(M)[0] for M in SIZES if M > 1}
    later = {R for M in SIZES for R in stages(M)[1:]}
    assert first == set(RADICES), sorted(set(RADICES) - first)
    assert later == set(RADICES), sorted(set(RADICES) - later)
    behind = {(p, R) for M in SIZES for p, R in zip(stages(M), stages(M)[1:]) if R in ODD}
    for R in ODD:
        prev = {p for p, r in behind if r == R}
        assert prev & set(ODD), R
    assert {R for p, R in behind if p == 2} >= {3, 7, 19, 23, 31}
    assert {R for p, R in behind if p == 4} >= {3, 7}


def test_stage_order_is_fft64s():
    assert stages(1) == []
    assert stages(8) == [4, 2]
    assert stages(12) == [4, 3]
    assert stages(612) == [4, 3, 3, 17]
    assert stages(1102) == [2, 19, 29]
    assert stages(2046) == [2, 3, 11, 31]
    assert stages(2048) == [4, 4, 4, 4, 4, 2]
    for M in SIZES:
        assert int(np.prod(stages(M), dtype=np.int64)) == M


@pytest.mark.parametrize("M", SIZES)
def test_reference_vs_numpy(M):
    """The long-double DFT against numpy's own fp64 FFT, an independent implementation: a
    wrong sign, index or root in the reference would show at O(1). 1e-15 is 4.5 units of
    fp64 rounding; numpy lies 1.0e-17 to 3.4e-16 from the reference over these sizes."""
    x, want = noise_case(M)
    assert rel_err(np.fft.fft(x), want[0]) <= 1e-15
    assert rel_err(np.fft.ifft(x) * M, want[1]) <= 1e-15


@pytest.mark.parametrize("M", SIZES)
def test_restatement_within_a_quarter_of_the_bound(M):
    x, want = noise_case(M)
    for inv in (False, True):
        e = rel_err(fft64_numpy(x, inv), want[inv])
        print("M %4d inv %d restatement err %.3g  TOL64 %.3g" % (M, inv, e, tol64(M)))
        assert e <= tol64(M) / 4, (M, inv, e, tol64(M))


@pytest.mark.parametrize("M", [37, 2049, 0, -4, 2 * 37, 1369])
def test_refusals_need_no_context(M):
    """The size check comes before the context is used: SG_E_UNSUPPORTED with ctx = NULL."""
    from soundgen_beta_amd import native
    assert native.lib().sg_debug_fft64(None, M, 0, 1, None, None) == -4


def test_null_context_is_an_argument_error():
    from soundgen_beta_amd import native
    buf = np.zeros(2 * 77)
    dp = C.POINTER(C.c_double)
    assert native.lib().sg_debug_fft64(None, 77, 0, 1, buf.ctypes.data_as(dp), buf.ctypes.data_as(dp)) == -1


# ---- GPU -------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    from soundgen_beta_amd import native
    c = native.Context(0)
    yield c
    c.close()


def gpu_fft64(ctx, x, inverse):
    from soundgen_beta_amd import native
    nf, M = x.shape
    src = np.ascontiguousarray(x, np.complex128).view(np.float64).ravel()
    dst = np.full_like(src, np.nan)
    dp = C.POINTER(C.c_double)
    native.check(native.lib().sg_debug_fft64(ctx.ptr, M, int(inverse), nf, src.ctypes.data_as(dp),
                                             dst.ctypes.data_as(dp)), ctx.ptr)
    return dst.view(np.complex128).reshape(nf, M)


@pytest.mark.gpu
@pytest.mark.parametrize("M", SIZES)
def test_fft64_vs_long_double(ctx, M):
    """Frame 0: noise. Frame 1: a unit impulse at index 1, whose transform is the root table.
    Frame 2: all ones, whose energy lands in bin 0. Both directions, no normalisation."""
    noise, want = noise_case(M)
    x = np.zeros((3, M), np.complex128)
    x[0] = noise
    x[1, 1 % M] = 1
    x[2] = 1
    tol = tol64(M)
    w = roots_ld(M)
    for inv in (0, 1):
        got = gpu_fft64(ctx, x, inv)
        assert np.isfinite(got.view(np.float64)).all(), (M, inv)
        e0 = rel_err(got[0], want[inv])
        e1 = rel_err(got[1], w.conj() if inv else w)
        d0 = abs(got[2, 0] - M)
        rest = float(np.abs(got[2, 1:]).max(initial=0.0))
        print("M %4d inv %d stages %s  noise %.3g  impulse %.3g  ones: bin0 %.3g rest %.3g  TOL64 %.3g"
              % (M, inv, stages(M), e0, e1, d0 / M, rest / M, tol))
        assert e0 <= tol, (M, inv, e0, tol)
        assert e1 <= tol, (M, inv, e1, tol)
        assert d0 <= tol * M, (M, inv, d0, tol * M)
        assert rest <= tol * M, (M, inv, rest, tol * M)


@pytest.mark.gpu
@pytest.mark.parametrize("M", [37, 2049, 0])
def test_refusals_leave_out_untouched(ctx, M):
    from soundgen_beta_amd import native
    n = 2 * max(M, 1)
    src = np.ones(n)
    dst = np.full(n, -7.25)
    dp = C.POINTER(C.c_double)
    rc = native.lib().sg_debug_fft64(ctx.ptr, M, 0, 1, src.ctypes.data_as(dp), dst.ctypes.data_as(dp))
    assert rc == -4
    assert (dst == -7.25).all()
