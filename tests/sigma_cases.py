"""The residual sets the robust-scale kernels (csrc/sigma_device.h, csrc/kernels_sigma.hip) are held to the oracle on: every sample count at which
the code takes another path, four scales, eight contaminations.  Plain numpy: no GPU, no torch.

Sample counts (COUNTS).  One workgroup of SIG_T = 512 threads serves a residual set; up to SIG_T * SIG_MAXPT = 20 480 samples a thread keeps its
ceil(n / 512) slots in registers, ROUNDED UP to a multiple of 8, above that it streams the array once per pass:
  63, 64, 65        one wave holds samples, seven hold padding only (64: exactly one wave)
  511, 512, 513     one slot per thread, a slot short, one over
  4096 g, 4096 g + 1 for g = 1..5: the last count of each slot group (8, 16, 24, 32, 40 slots) and the first of the next; 20 480 / 20 481 is the switch
                    from the register path to the streaming one
  20 991, 24 577    streaming; 20 991 = 41 * 512 - 1 leaves a ragged last stride
  1, 2, 3           degenerate: sigma = 0 after the first pass (n = 1), or a scale from two or three samples

Scales (SCALES) as (sigma, bias, start sigma): the inverse-depth channel's (0.004, 0.0005, 0.0025), the intensity channel's (7, -1, 5), (2, 6, 5)
with a bias of three sigma, and (3.9, 0.5, 5): the least-squares sigma of the first pass, sqrt(5 / 3) * 3.9 = 5.03, lies within 10 % of the start value, so
a stop test evaluated after the first pass already (it must not be) would end the loop there -- no other scale would show that.  The start bias is 0
everywhere, as the tracker sets it.  The start sigmas are the two `rgbid_sigma_pair_batched` uses.

Contaminations (CONTAMINATIONS) of bias + sigma * t_5: see residuals().

LEFT OUT ON PURPOSE: 1e30 outliers in computeSigmaAndNuStudent / computeSigmaPdf.  The reference's own fp32 first pass overflows on them (e * e =
inf): the oracle returns sigma = inf and nu = 10 with a bias that depends on the order of summation -- nothing can be held to that.  computeNuStudent,
which takes bias and sigma from its caller, is held to 1e30 outliers in tests/test_gpu_kfalign.py (kfalign_cases `huge`).

A case is DECIDED for an entry point when the reference's answer is not sitting on one of its own discontinuities (decided_student / decided_pdf).
"""
import functools

import numpy as np

from tests import np_mirror as M

SEED = 20261020
CASE_SEED = 0      # chosen on the CPU (tests/test_cpu_sigma_cases.py): at most 1 case in 20 undecided per entry point
# Seeds of the degenerate counts, chosen on the CPU by a condition on the REFERENCE alone (tests/test_cpu_sigma_cases.py asserts it): the first seed at which
# the oracle and its float64 mirror agree to a tenth of the device bar on every finite result of every set at that count.  With two or three samples whose
# spread is a few per cent of their mean the reference's fp32 reduction swsr - 2 b swr + b^2 sw cancels to its last bits (seed 0: oracle and mirror 1.7e-3
# sigma apart at n = 2), and logf(1 + en^2 / 5) of a single small en carries the rounding of 1 + x: no bar on a third implementation means anything there.
SEEDS = {1: 3, 2: 8, 3: 1}
SIG_T, SIG_MAXPT = 512, 40
REG_MAX = SIG_T * SIG_MAXPT
DEGENERATE = (1, 2, 3)
COUNTS = (63, 64, 65, 511, 512, 513) + tuple(4096 * g + d for g in range(1, 6) for d in (0, 1)) + (20991, 24577) + DEGENERATE
SCALES = ((0.004, 0.0005, 0.0025), (7.0, -1.0, 5.0), (2.0, 6.0, 5.0), (3.9, 0.5, 5.0))
CONTAMINATIONS = ("clean", "nan30", "nan90", "nan100", "inf", "wild", "tail", "shift")
LSQ, HUBER, TUKEY, STUDENT = range(4)
MESTIMATORS = (LSQ, HUBER, TUKEY, STUDENT)
NU_GRID = tuple(2.0 + 0.25 * k for k in range(33))    # every value the bisection on [2, 10] can return (its last midpoints are multiples of 0.25)
STOP, NEAR_STOP, PERTURB = 0.1, 1e-3, 1e-5


def path(n):
    return "register" if n <= REG_MAX else "streaming"


def slots(n):
    """slots per thread the register path's passes visit"""
    return (-(-n // SIG_T) + 7) & ~7


@functools.lru_cache(maxsize=None)
def residuals(n, scale, contamination, seed=None):
    """bias + sigma * t_5, float32 [n], read-only, with
      clean    nothing
      nan30    30 % NaN
      nan90    90 % NaN: at n = 64 half a dozen valid samples among 4 096 register slots
      nan100   all NaN
      inf      max(2, n / 200) samples set to alternating -+inf
      wild     as many at bias -+ 1e4 sigma: the IRLS loop needs 7 passes or runs into its cap of 10
      tail     the last eighth times 4 (4-5 passes; a kernel that drops the end of the array sees another distribution)
      shift    every third sample + 3 sigma (2 passes)
    `scale` indexes SCALES."""
    sigma, bias, _ = SCALES[scale]
    seed = SEEDS.get(n, CASE_SEED) if seed is None else seed
    r = np.random.default_rng([SEED, n, scale, CONTAMINATIONS.index(contamination), seed])
    e = (bias + sigma * r.standard_t(5.0, n)).astype(np.float32)
    k = min(n, max(2, n // 200))
    few = r.choice(n, k, replace=False)
    odd = (np.arange(k) & 1).astype(bool)
    if contamination == "nan30":
        e[r.random(n) < 0.3] = np.nan
    elif contamination == "nan90":
        e[r.random(n) < 0.9] = np.nan
    elif contamination == "nan100":
        e[:] = np.nan
    elif contamination == "inf":
        e[few] = np.where(odd, np.inf, -np.inf).astype(np.float32)
    elif contamination == "wild":
        e[few] = (bias + np.where(odd, 1e4, -1e4) * sigma).astype(np.float32)
    elif contamination == "tail":
        e[n - n // 8:] *= np.float32(4.0)
    elif contamination == "shift":
        e[::3] += np.float32(3.0 * sigma)
    else:
        assert contamination == "clean"
    e.setflags(write=False)
    return e


def cases(n):
    """-> ((scale index, contamination, residuals), ...) at one sample count"""
    return tuple((s, c, residuals(n, s, c)) for s in range(len(SCALES)) for c in CONTAMINATIONS)


def start_sigma(scale):
    return SCALES[scale][2]


def chi_pairs(n):
    """computeChiSquare takes both channels at once: the intensity-scale set and the inverse-depth-scale set of one contamination, normalised by the sigmas
    they were drawn with -> ((contamination, err_int, err_depth, sigma_int, sigma_depth), ...)"""
    return tuple((c, residuals(n, 1, c), residuals(n, 0, c), SCALES[1][0], SCALES[0][0]) for c in CONTAMINATIONS)


def _near_stop(ratios):
    return any(abs(r - STOP) < NEAR_STOP for r in ratios)     # a NaN ratio fails the reference's `<` in every arithmetic: not near


def passes_student(e, s0, mestimator=STUDENT):
    """-> the stop-test ratios of the float64 mirror's computeSigmaAndNuStudent loop (one per pass after the first)"""
    t = []
    with np.errstate(all="ignore"):
        M.sigma_nu_student(e, 0.0, s0, mestimator, trace=t)
    return t


def decided_student(sigma_nu_of, e, s0, mestimator=STUDENT):
    """computeSigmaAndNuStudent on residuals e from (bias 0, sigma s0).  The pass count is a discontinuous function of the residuals where the stop test's
    ratio |sigma - sigma_prev| / sigma_prev sits on its threshold 0.1, and nu is a value of the bisection grid that a sum a few ulp off can move by
    a step.  DECIDED: (a) no pass of the float64 mirror has that ratio within 1e-3 of 0.1, and (b) the reference sigma_nu_of(e, bias, sigma, nu, mest)
    gives the same nu for e, e (1 + 1e-5) and e (1 - 1e-5) (kfalign_cases.nu_decided's idea).  -> (decided, near_stop, nu_moves)"""
    near = _near_stop(passes_student(e, s0, mestimator))
    with np.errstate(all="ignore"):
        nus = [sigma_nu_of(e * np.float32(f), 0.0, s0, 5.0, mestimator)[2] for f in (1.0, 1.0 + PERTURB, 1.0 - PERTURB)]
    moves = not (nus[0] == nus[1] == nus[2])
    return (not near and not moves), near, moves


def decided_nu(nu_of, e, bias, sigma):
    """computeNuStudent at a given bias and scale: decided when the reference nu_of(e, bias, sigma) gives the same nu for e, e (1 + 1e-5) and e (1 - 1e-5)
    -> (nu, decided)"""
    with np.errstate(all="ignore"):
        nus = [nu_of(e * np.float32(f), bias, sigma) for f in (1.0, 1.0 + PERTURB, 1.0 - PERTURB)]
    return nus[0], nus[0] == nus[1] == nus[2]


def decided_pdf(e, s0, mestimator):
    """computeSigmaPdf: only the stop test is discontinuous -> decided"""
    t = []
    with np.errstate(all="ignore"):
        M.sigma_pdf(e, 0.0, s0, mestimator, trace=t)
    return not _near_stop(t)


def same_nonfinite(got, ref):
    """NaN for NaN, an inf of the same sign for inf"""
    if np.isnan(ref):
        return bool(np.isnan(got))
    return bool(np.isinf(got)) and (got > 0) == (ref > 0)


def bits(*values):
    """float32 bit patterns: equality that tells NaN from NaN payloads apart and -0 from 0"""
    return tuple(int(np.float32(v).view(np.uint32)) for v in values)
