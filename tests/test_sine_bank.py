"""The six sine-bank kernels (sg_harm.hip) task by task, through the hook sg_debug_sine_bank:
the product's classifier and launchers on tasks this file builds, every sample against a
direct long-double evaluation of the task's sum

    m = mbase + l,  P = c0 + m (c1 + m (c2 + m (c3 + m c4))),  t = (tc0 + l xby) rdx  (0: CONST)
    W(l) = sum_{r = 1..Rn} (A_r + t (A1_r - A_r)) sin(2 pi r (P - rint P))

at the smallest shapes that reach each path of each kernel (BUILDERS below, one hook call per class).

The bound is not fitted to the kernels. Per class, a sample's deviation from the reference
divided by its sum_r |a_r| may be 8 times the largest such deviation of a numpy restatement
of the class's algorithm in the class's precision (plain Clenshaw in fp32 for sg_sine_bank,
_pairs and _tab; Clenshaw in fp64, rounded to fp32, for _tall and unrounded for _hp; Reinsch's
form in fp32 for _tall_pairs), over every task of the class in this file. 8 is the margin
tests/test_formants.py gives the GPU over its host restatement. The table class adds
SG_TAB_TOL, the project's own interpolation bound. The fp64 class keeps one bound for its
CONST tasks and one for the others, whose fp32 weight t dominates: a finer partition, so
never a wider bound.

Table columns: a job's column must meet the planner's criterion
(2 pi)^4 sum |A_r| r^4 / (384 N^4) <= SG_TAB_TOL sum |A_r| for the test to hold the job to
SG_TAB_TOL, so Rn = 96 (|A_r| = 1 / r^2) runs at logn 11 only, Rn = 4 at 8 and 11."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

LD = np.longdouble
F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "soundgen_beta_amd", "csrc")

CONST, LIN, ENV, HP = 1, 2, 4, 8
TASK_MAX, RUN_TASKS, ROWS_F32 = 1024, 8, 96
TAB_TASKS, TAB_LOGN_MIN, TAB_LOGN_MAX, TAB_TOL = 64, 8, 11, 1e-7
LONG, PAIRS, TALL, TALL_PAIRS, HPC, TABLE = range(6)
CLASS_NAMES = ("long", "pairs", "tall", "tall_pairs", "hp", "table")
FACTOR = 8.0
ENV_VALUE = 0.8125
SR = 44100.0


class SgWTask(C.Structure):
    _fields_ = [("w_off", C.c_int64), ("a_off", C.c_int64), ("d_off", C.c_int64), ("dk0", C.c_int64),
                ("c0", C.c_double), ("c1", C.c_double), ("c2", C.c_double), ("c3", C.c_double),
                ("c4", C.c_double), ("invD", C.c_double),
                ("rdx", C.c_float), ("tc0", C.c_float), ("xby", C.c_float),
                ("mbase", C.c_int32), ("R", C.c_int32), ("j0", C.c_int32), ("len", C.c_int32),
                ("dj0", C.c_int32), ("dj1", C.c_int32), ("syl", C.c_int32), ("flags", C.c_int32),
                ("Rn", C.c_int32)]


class SgTabJob(C.Structure):
    _fields_ = [("a_off", C.c_int64), ("Rn", C.c_int32), ("t0", C.c_int32), ("n", C.c_int32),
                ("logn", C.c_int32), ("syl", C.c_int32), ("flags", C.c_int32)]


TASK = np.dtype(SgWTask)
JOB = np.dtype(SgTabJob)


# ---- cases -----------------------------------------------------------------

class Builder:
    """Tasks of one hook call: amplitude columns, a scratch with gaps between the tasks."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.tasks, self.want, self.jobs = [], [], []
        self.amps = [np.zeros(5, F32)]  # a column never starts at 0
        self.namps = 5
        self.cur = 19
        self.cols = {}

    def column(self, R, Rn, power):
        """Two columns of R rows: |A_r| = r^-power with random signs for r <= Rn, 0 above;
        A1 = A + dA with |dA_r| between 0.25 and 0.4 of |A_r|, random signs."""
        key = (R, Rn, power)
        if key not in self.cols:
            rng = np.random.default_rng([R, Rn, int(power * 8)])
            r = np.arange(1, R + 1, dtype=np.float64)
            A = np.where(r <= Rn, rng.choice([-1.0, 1.0], R) / r ** power, 0.0).astype(F32)
            dA = rng.choice([-1.0, 1.0], R) * rng.uniform(0.25, 0.4, R) * np.abs(A)
            A1 = (A + dA).astype(F32)
            self.cols[key] = (self.namps, self.namps + R)
            self.amps += [A, A1]
            self.namps += 2 * R
        return self.cols[key]

    def task(self, want, n, R, Rn, flags, window, syl, cubic=False, power=1.0, f=None):
        rng = self.rng
        a_off, d_off = self.column(R, Rn, power)
        t = np.zeros((), TASK)
        j0 = int(rng.integers(0, 400))
        t["w_off"], t["j0"], t["len"] = self.cur - j0, j0, n
        self.cur += n + int(rng.integers(1, 70))
        t["a_off"], t["d_off"], t["R"], t["Rn"] = a_off, d_off, R, Rn
        t["dk0"] = int(rng.integers(0, 5000))
        f = float(np.exp(rng.uniform(np.log(50.0), np.log(9000.0)))) if f is None else f
        t["c0"], t["c1"] = rng.uniform(0, 1), f / SR
        if cubic:
            assert not flags & LIN
            t["c2"] = rng.choice([-1, 1]) * rng.uniform(0.5e-9, 2e-9)
            t["c3"] = rng.choice([-1, 1]) * rng.uniform(0.5e-15, 2e-15)
            t["c4"] = rng.choice([-1, 0, 1]) * rng.uniform(0.5e-21, 2e-21)
        t["invD"] = 1.0
        t["mbase"] = int(rng.integers(0, 100000))
        # the approx() weight runs from tc0 rdx in steps of xby rdx; a CONST task carries
        # the fields too, and the kernels must not look at them
        step = max(1.0 / n, 1.0 / 256)
        t["rdx"] = rng.uniform(0.5, 2.0)
        t["xby"] = step / float(t["rdx"])
        t["tc0"] = rng.uniform(0.0, 0.3) / float(t["rdx"])
        cut = (n // 2) | 1  # odd: in the middle of a pass, never on a slot boundary
        lo, hi = max(0, j0 - 5), j0 + n + 9
        t["dj0"], t["dj1"] = {"whole": (lo, hi), "low": (j0 + cut, hi), "high": (lo, j0 + cut),
                              "empty": (j0 + n // 2, j0 + n // 2)}[window]
        t["syl"], t["flags"] = syl, flags
        if n <= 2:
            # one or two samples could sit where a mutation of the reference (reference()) hardly
            # moves it, and a kernel wrong in that way would go unseen: of 32 starting phases,
            # the one at which the least of the mutations moves the reference most
            amps = np.concatenate(self.amps)
            best = []
            for k in range(32):
                t["c0"] = (k + rng.uniform(0, 1)) / 32
                best.append((min(reference(t, amps)[2].values()), float(t["c0"])))
            t["c0"] = max(best)[1]
        self.tasks.append(t)
        self.want.append(want)
        return len(self.tasks) - 1

    def job(self, t0, n, logn):
        j = np.zeros((), JOB)
        t = self.tasks[t0]
        j["a_off"], j["Rn"], j["t0"], j["n"], j["logn"] = t["a_off"], t["Rn"], t0, n, logn
        self.jobs.append(j)

    def done(self):
        return (np.array([t[()] for t in self.tasks], TASK), np.array(self.want, np.int32),
                np.concatenate(self.amps), self.cur + 23, np.array([j[()] for j in self.jobs], JOB))


WINDOWS = ("whole", "low", "high", "empty")
ROWS_LONG = (4, 8, 12, 16, 92, 96)


def rows_long(Rn, wide):
    """R of a long-class task: 16 or 96; Rn < R at 4, 8, 12 and 92, and at 16 when wide."""
    return 96 if Rn > 16 or wide else 16


def build_long():
    b = Builder(1)
    k = 0
    for i, n in enumerate((65, 128, 129, 192, 193, 256, 257, 448, 449, 512, 513, 960, 1024)):  # CONST
        for q, Rn in enumerate(ROWS_LONG):
            for lin in (0, 1):
                b.task(LONG, n, rows_long(Rn, lin), Rn, CONST | (LIN if lin else 0), WINDOWS[(i + q + lin) % 4],
                       syl=k // 3, cubic=not lin and q % 2 == 1)
                k += 1
    for i, n in enumerate((65, 193, 257, 1024)):  # two columns: linear (flagged) and cubic phase
        for q, Rn in enumerate(ROWS_LONG):
            for lin in (0, 1):
                b.task(LONG, n, rows_long(Rn, not lin), Rn, LIN if lin else 0, WINDOWS[(i + q + lin) % 4],
                       syl=1000 + k // 3, cubic=not lin)
                k += 1
    for i, n in enumerate((1, 64, 65, 300)):  # amplitude envelope
        for q, Rn in enumerate(ROWS_LONG):
            for const in (0, 1):
                b.task(LONG, n, rows_long(Rn, const), Rn, ENV | (CONST if const else 0),
                       WINDOWS[(i + q + const) % 4], syl=2000 + k // 2, cubic=q % 2 == 0)
                k += 1
    return b.done()


def build_pairs():
    """Syllables of 1, 2, 3, 8, 9 and 17 tasks (runs of at most SG_RUN_TASKS, an odd last task
    pairs with itself), twice with the cycles shifted: partners with R 16 / 96, CONST / not,
    one window whole and the other empty."""
    b = Builder(2)
    lens, rows = (64, 1, 63, 2), (4, 96, 8, 92, 12, 48, 16, 20)
    k = 0
    for rep in (0, 1):
        for s, nt in enumerate((1, 2, 3, 8, 9, 17)):
            for i in range(nt):
                Rn = rows[(k + rep) % 8]
                const = CONST if (k // 2 + k // 3 + rep) % 2 else 0
                lin = LIN if k % 5 == 0 else 0
                b.task(PAIRS, lens[(k + 3 * rep) % 4], 16 if Rn <= 16 else 96, Rn, const | lin,
                       ("whole", "empty")[(i + s + rep) % 2], syl=10 * rep + s, cubic=not lin and k % 2 == 0)
                k += 1
    return b.done()


def rows_tall(Rn):
    return max(112, (Rn + 15) // 16 * 16)


def build_tall():
    b = Builder(3)
    k = 0
    for i, n in enumerate((1, 65, 128, 129, 1024)):
        for q, Rn in enumerate((4, 100, 112, 256, 260, 512, 516)):
            flags = (CONST if (i + q) % 2 else 0) | (ENV if n == 1 or (i + q) % 5 == 0 else 0)
            b.task(TALL, n, rows_tall(Rn), Rn, flags, WINDOWS[(i + q) % 4], syl=k // 2, cubic=k % 2 == 0)
            k += 1
    return b.done()


def build_tall_pairs():
    """Runs of 1, 3, 8 and 9 (8 + 1) tasks, twice: partners with different Rn, 128-row chunks."""
    b = Builder(4)
    rows = (100, 260, 112, 144, 128, 132)
    k = 0
    for rep in (0, 1):
        for s, nt in enumerate((1, 3, 8, 9)):
            for i in range(nt):
                Rn = rows[(k + rep) % 6]
                b.task(TALL_PAIRS, (1, 64)[(k + k // 3) % 2], rows_tall(Rn), Rn, CONST if (k // 2 + rep) % 2 else 0,
                       ("whole", "empty", "low")[(i + s) % 3], syl=10 * rep + s, cubic=k % 2 == 1)
                k += 1
    return b.done()


def build_hp():
    b = Builder(5)
    k = 0
    for i, n in enumerate((1, 65, 128, 129, 1024)):
        for q, (R, Rn) in enumerate(((16, 12), (16, 16), (96, 92), (96, 96), (112, 100), (112, 112))):
            for lin in (0, 1):
                env = ENV if not lin and (i + q) % 3 == 0 else 0
                b.task(HPC, n, R, Rn, HP | env | (LIN if lin else 0) | (CONST if (i + q + lin) % 2 else 0),
                       WINDOWS[(i + q + lin) % 4], syl=k // 2, cubic=not lin)
                k += 1
    return b.done()


def build_table():
    """Jobs of 1, 8 and 64 tasks; two CONST | LIN tasks outside every job stay on the recurrence."""
    b = Builder(6)
    lens = (1, 63, 255, 256, 257, 1024)
    t0 = b.task(TABLE, 1024, 16, 4, CONST | LIN, "low", syl=0, f=431.0)  # the window cuts a 256-block
    b.job(t0, 1, 8)
    b.task(LONG, 257, 16, 4, CONST | LIN, "whole", syl=0, f=431.0)
    first = len(b.tasks)
    for i in range(8):
        b.task(TABLE, (lens + (256, 1024))[i], 96, 96, CONST | LIN, WINDOWS[i % 4], syl=1, power=2.0, f=97.0)
    b.job(first, 8, 11)
    first = len(b.tasks)
    for i in range(64):
        b.task(TABLE, lens[i % 6], 16, 4, CONST | LIN, WINDOWS[(i // 6) % 4], syl=2 + i // 40, f=1234.5)
    b.job(first, 64, 11)
    b.task(LONG, 300, 96, 96, CONST | LIN, "high", syl=4, power=2.0, f=97.0)
    t0 = b.task(TABLE, 257, 96, 96, CONST | LIN, "high", syl=5, power=2.0, f=55.0)
    b.job(t0, 1, 11)
    first = len(b.tasks)
    for i in range(8):
        b.task(TABLE, lens[(i + 2) % 6], 96, 4, CONST | LIN, WINDOWS[(i + 1) % 4], syl=6, f=3000.0)
    b.job(first, 8, 8)
    return b.done()


BUILDERS = {"long": build_long, "pairs": build_pairs, "tall": build_tall, "tall_pairs": build_tall_pairs,
            "hp": build_hp, "table": build_table}


# ---- reference and restatements ---------------------------------------------

def _pi():
    return LD(4) * np.arctan(LD(1))


def reference(t, amps):
    """The direct long-double sum of one task and its three mutations' largest normalised
    deviations: sample l + 1 in place of l, t one step further, the top four rows dropped."""
    n, Rn = int(t["len"]), int(t["Rn"])
    l = np.arange(n + 1).astype(LD)
    m = LD(int(t["mbase"])) + l
    c = [LD(float(t["c%d" % k])) for k in range(5)]
    P = c[0] + m * (c[1] + m * (c[2] + m * (c[3] + m * c[4])))
    x = P - np.rint(P)
    A = amps[int(t["a_off"]):int(t["a_off"]) + Rn].astype(LD)
    dA = amps[int(t["d_off"]):int(t["d_off"]) + Rn].astype(LD) - A
    const = bool(t["flags"] & CONST)
    step = LD(float(t["xby"])) * LD(float(t["rdx"]))
    tt = np.zeros(n + 1, LD) if const else (LD(float(t["tc0"])) + l * LD(float(t["xby"]))) * LD(float(t["rdx"]))
    S = np.sin((LD(2) * _pi()) * np.outer(x, np.arange(1, Rn + 1).astype(LD)))
    a = A[None, :] + tt[:, None] * dA[None, :]
    ref = (S[:n] * a[:n]).sum(1)
    norm = np.abs(a[:n]).sum(1)
    mut = {"shift": float((np.abs((S[1:] * a[1:]).sum(1) - ref) / norm).max()),
           "top4": float((np.abs((S[:n, Rn - 4:] * a[:n, Rn - 4:]).sum(1)) / norm).max())}
    if not const:
        mut["t"] = float((np.abs(step * (S[:n] * dA[None, :]).sum(1)) / norm).max())
    return ref, norm, mut


def _phase64(t):
    m = (int(t["mbase"]) + np.arange(int(t["len"]))).astype(np.float64)
    c = [float(t["c%d" % k]) for k in range(5)]
    P = c[0] + m * (c[1] + m * (c[2] + m * (c[3] + m * c[4])))
    return P - np.rint(P)


def _weight32(t):
    n = int(t["len"])
    if t["flags"] & CONST:
        return np.zeros(n, F32)
    return (np.arange(n).astype(F32) * F32(t["xby"]) + F32(t["tc0"])) * F32(t["rdx"])


def _columns32(t, amps):
    Rn = int(t["Rn"])
    A = amps[int(t["a_off"]):int(t["a_off"]) + Rn]
    return A, amps[int(t["d_off"]):int(t["d_off"]) + Rn] - A  # the difference formed in fp32, as staged


def clenshaw32(t, amps):
    """b_r = a_r + 2 cos(theta) b_{r+1} - b_{r+2}, W = b_1 sin(theta), all in fp32; the cycle
    fraction reduced in fp64 and rounded to fp32, sin and cos correctly rounded."""
    A, dA = _columns32(t, amps)
    x = _phase64(t).astype(F32)
    th = 2.0 * np.pi * x.astype(np.float64)
    sn, al = np.sin(th).astype(F32), (2.0 * np.cos(th)).astype(F32)
    tt = _weight32(t)
    b1 = np.zeros_like(x)
    b2 = np.zeros_like(x)
    for r in range(len(A) - 1, -1, -1):
        b1, b2 = al * b1 + ((A[r] + tt * dA[r]) - b2), b1
    assert b1.dtype == F32
    return (b1 * sn).astype(np.float64)


def clenshaw64(t, amps):
    """The same recurrence in fp64 on the fp64 cycle fraction; t in fp32."""
    A, dA = _columns32(t, amps)
    A, dA = A.astype(np.float64), dA.astype(np.float64)
    th = 2.0 * np.pi * _phase64(t)
    sn, al = np.sin(th), 2.0 * np.cos(th)
    tt = _weight32(t).astype(np.float64)
    b1 = np.zeros_like(th)
    b2 = np.zeros_like(th)
    for r in range(len(A) - 1, -1, -1):
        b1, b2 = al * b1 + ((A[r] + tt * dA[r]) - b2), b1
    return b1 * sn


def reinsch32(t, amps):
    """Reinsch's form in fp32: d_k = a_k + u b_{k+1} + sg d_{k+1}, b_k = d_k + sg b_{k+1},
    W = b_1 sin(theta), sg = sign cos(theta), u = -4 sin^2(theta / 2) or 4 cos^2(theta / 2);
    the half angle's sine and cosine correctly rounded to fp32."""
    A, dA = _columns32(t, amps)
    x = _phase64(t).astype(F32)
    h = (F32(np.pi) * x).astype(np.float64)
    s, c = np.sin(h).astype(F32), np.cos(h).astype(F32)
    sn = F32(2) * s * c
    pos = np.abs(x) <= F32(0.25)
    sg = np.where(pos, F32(1), F32(-1))
    u = np.where(pos, F32(-4) * s * s, F32(4) * c * c)
    tt = _weight32(t)
    b = np.zeros_like(x)
    d = np.zeros_like(x)
    for r in range(len(A) - 1, -1, -1):
        d = ((A[r] + tt * dA[r]) + u * b) + sg * d
        b = d + sg * b
    assert b.dtype == F32
    return (b * sn).astype(np.float64)


def restate(cls, t, amps):
    if cls in (LONG, PAIRS, TABLE):
        return clenshaw32(t, amps)
    if cls == TALL:
        return clenshaw64(t, amps).astype(F32).astype(np.float64)
    if cls == HPC:
        return clenshaw64(t, amps)
    return reinsch32(t, amps)


def bound_key(cls, t):
    """The class; the fp64 class apart for CONST tasks (module docstring)."""
    return (cls, bool(t["flags"] & CONST)) if cls == HPC else (cls, None)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(name):
    """One hook call's inputs with each task's reference, norm, mutations and restatement
    deviation: computed once, shared by the CPU and the GPU tests, never written to."""
    c = Case()
    c.name = name
    c.tasks, c.want, c.amps, c.wlen, c.jobs = BUILDERS[name]()
    c.ref, c.norm, c.mut, c.rdev = [], [], [], []
    for t, cls in zip(c.tasks, c.want):
        ref, norm, mut = reference(t, c.amps)
        dev = np.abs(restate(int(cls), t, c.amps).astype(LD) - ref) / norm
        for v in (ref, norm):
            v.setflags(write=False)
        c.ref.append(ref)
        c.norm.append(norm)
        c.mut.append(mut)
        c.rdev.append(float(dev.max()))
    for v in (c.tasks, c.want, c.amps, c.jobs):
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def measured():
    """Per bound key the largest normalised deviation of the class's restatement over every
    task of the class in this file."""
    out = {}
    for name in BUILDERS:
        c = case(name)
        for t, cls, d in zip(c.tasks, c.want, c.rdev):
            k = bound_key(int(cls), t)
            out[k] = max(out.get(k, 0.0), d)
    return out


def bound(cls, t):
    return FACTOR * measured()[bound_key(cls, t)] + (TAB_TOL if cls == TABLE else 0.0)


# ---- CPU ---------------------------------------------------------------------

def test_long_double_is_wider_than_double():
    assert np.finfo(LD).eps <= 2.0 ** -63


def test_layout_matches_the_headers(tmp_path):
    """sizeof and every offsetof of SgWTask and SgTabJob, and the constants this file restates,
    from a stand-alone g++ program that includes sg_dev.h, against the ctypes mirrors."""
    exe = str(tmp_path / "sine_bank_layout")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I" + CSRC, os.path.join(HERE, "cpp", "sine_bank_layout.cpp"),
                    "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout
    got = {"SgWTask": [], "SgTabJob": []}
    consts = {}
    for line in out.splitlines():
        a, b, v = line.split()
        if a == "const":
            consts[b] = float(v)
        else:
            got[a].append((b, int(v)))
    for S in (SgWTask, SgTabJob):
        want = [("sizeof", C.sizeof(S))] + [(f, getattr(S, f).offset) for f, _ in S._fields_]
        assert got[S.__name__] == want
    assert C.sizeof(SgWTask) == 128 and TASK.itemsize == 128 and JOB.itemsize == C.sizeof(SgTabJob) == 32
    assert consts == dict(SG_TASK_CONST=CONST, SG_TASK_LIN=LIN, SG_TASK_ENV=ENV, SG_TASK_HP=HP, SG_TASK_MAX=TASK_MAX,
                          SG_RUN_TASKS=RUN_TASKS, SG_ROWS_F32=ROWS_F32, SG_TAB_TASKS=TAB_TASKS,
                          SG_TAB_LOGN_MIN=TAB_LOGN_MIN, SG_TAB_LOGN_MAX=TAB_LOGN_MAX, SG_TAB_TOL=TAB_TOL)


def classify(tasks, jobs):
    """classify_block (sg_exec.cpp) restated: the class every task is meant to reach."""
    out = []
    in_tab = set(int(q) for j in jobs for q in range(int(j["t0"]), int(j["t0"]) + int(j["n"])))
    for i, t in enumerate(tasks):
        short = t["len"] <= 64 and not t["flags"] & ENV
        out.append(TABLE if i in in_tab else HPC if t["flags"] & HP else
                   (TALL_PAIRS if short else TALL) if t["R"] > ROWS_F32 else PAIRS if short else LONG)
    return np.array(out, np.int32)


def passes(t):
    """The slot counts of run_task's passes over a task (sg_harm.hip), in order."""
    n, l0, out = int(t["len"]), 0, []
    if t["flags"] & HP or t["R"] > ROWS_F32:
        while n - l0 > 64:
            out.append(2)
            l0 += 128
        return out + ([1] if l0 < n else [])
    if t["flags"] & CONST:
        while n - l0 > 448:
            out.append(8)
            l0 += 512
    while n - l0 > 192:
        out.append(4)
        l0 += 256
    if n - l0 > 64:
        out.append(2)
        l0 += 128
    return out + ([1] if l0 < n else [])


def test_cases_reach_every_path():
    """The shapes the kernels branch on, from the records alone: every class as intended, every
    pass width of the fp32 and the fp64 tasks, the rotation shortcut, the n & 4 top group and
    its absence, staged rows and 256-row chunks, passes wholly inside and cut by the window,
    run lengths 1 .. SG_RUN_TASKS with odd last tasks, unequal and CONST / non-CONST partners."""
    for name in BUILDERS:
        c = case(name)
        assert (classify(c.tasks, c.jobs) == c.want).all(), name
        assert len(c.tasks) <= 400, name
    lg = case("long")
    f32 = [passes(t) for t in lg.tasks if not t["flags"] & ENV]
    assert {w for p in f32 for w in p} == {8, 4, 2, 1}
    assert {tuple(passes(t)) for t in lg.tasks if t["flags"] & CONST and not t["flags"] & ENV} >= {
        (2,), (2, 1), (4,), (4, 1), (4, 2, 1), (8,), (8, 1), (8, 4, 2, 1), (8, 8)}
    assert any(t["flags"] & LIN and not t["flags"] & CONST and passes(t)[0] == 4 for t in lg.tasks)  # rotation, two columns
    assert {int(t["Rn"]) & 4 for t in lg.tasks} == {0, 4}
    tl = case("tall")
    assert {int(t["Rn"]) > 256 for t in tl.tasks} == {False, True}
    assert {w for t in tl.tasks for w in passes(t)} == {2, 1}
    for c in (lg, tl, case("hp")):
        kinds = set()
        for t in c.tasks:
            l0 = 0
            for w in passes(t):
                a, b = int(t["j0"]) + l0, int(t["j0"]) + l0 + 64 * w
                full = l0 + 64 * w <= t["len"] and a >= t["dj0"] and b <= t["dj1"] and not t["flags"] & ENV
                kinds.add("inside" if full else "cut" if a < t["dj1"] and b > t["dj0"] and t["dj1"] > t["dj0"] else "outside")
                l0 += 64 * w
        assert kinds == {"inside", "cut", "outside"}, c.name
    for name, sizes in (("pairs", {1, 2, 3, 8}), ("tall_pairs", {1, 3, 8})):
        c = case(name)
        runs, pairs = [], set()
        for i, t in enumerate(c.tasks):
            if i == 0 or t["syl"] != c.tasks[i - 1]["syl"] or len(runs[-1]) == RUN_TASKS:
                runs.append([])
            runs[-1].append(i)
        assert {len(r) for r in runs} >= sizes, name
        for r in runs:
            for k in range(0, len(r), 2):
                p, q = c.tasks[r[k]], c.tasks[r[min(k + 1, len(r) - 1)]]
                pairs.add((bool(p["flags"] & CONST), bool(q["flags"] & CONST), int(np.sign(int(p["Rn"]) - int(q["Rn"])))))
        assert {(a, b) for a, b, _ in pairs} == {(False, False), (False, True), (True, False), (True, True)}, name
        assert {s for _, _, s in pairs} == {-1, 0, 1}, name
    tp = case("tall_pairs")
    assert any(t["Rn"] > 128 and t["Rn"] % 128 for t in tp.tasks)  # two chunks, the top one partial
    tb = case("table")
    assert sorted({(int(j["n"]), int(j["logn"])) for j in tb.jobs}) == [(1, 8), (1, 11), (8, 8), (8, 11), (64, 11)]
    assert (tb.want == LONG).sum() == 2


def test_bound_is_measured():
    """Prints, per class, the largest normalised deviation of its restatement from the
    long-double sum over the class's tasks here; the GPU may deviate FACTOR = 8 times as far
    (the table class: plus SG_TAB_TOL). The values must be positive and at most 1e-5.

    Measured (x86-64, 80-bit long double):
      long        fp32 Clenshaw                     2.30e-06   bound 1.84e-05
      pairs       fp32 Clenshaw                     3.80e-07   bound 3.04e-06
      tall        fp64 Clenshaw rounded to fp32     1.40e-07   bound 1.12e-06
      tall_pairs  fp32 Reinsch                      1.15e-06   bound 9.18e-06
      hp          fp64 Clenshaw, two columns        8.72e-08   bound 6.98e-07
      hp          fp64 Clenshaw, CONST              2.49e-11   bound 2.00e-10
      table       fp32 Clenshaw (+ SG_TAB_TOL)      1.76e-07   bound 1.51e-06"""
    m = measured()
    for (cls, const), v in sorted(m.items(), key=lambda kv: (kv[0][0], str(kv[0][1]))):
        print("class %-10s %-9s restatement %.3g  bound %.3g" % (
            CLASS_NAMES[cls], {None: "", True: "CONST", False: "two-column"}[const], v,
            FACTOR * v + (TAB_TOL if cls == TABLE else 0)))
    assert set(k[0] for k in m) == set(range(6))
    assert all(0 < v <= 1e-5 for v in m.values()), m


def test_cases_are_well_conditioned():
    """From the reference and the restatements alone, over every task of every case: the
    restatement's normalised deviation is positive and at most 1e-5; |dA_r| >= 0.2 |A_r| on the
    two-column tasks; rows Rn .. R of both columns are zero; each mutation of the reference
    (sample l + 1 for l, t one step of xby rdx further, the top four rows dropped) moves it by
    at least 10 times the task's bound; a table job's column meets the planner's criterion."""
    for name in BUILDERS:
        c = case(name)
        for i, (t, cls) in enumerate(zip(c.tasks, c.want)):
            where = (name, i)
            assert 0 < c.rdev[i] <= 1e-5, (where, c.rdev[i])
            R, Rn = int(t["R"]), int(t["Rn"])
            A = c.amps[int(t["a_off"]):int(t["a_off"]) + R]
            A1 = c.amps[int(t["d_off"]):int(t["d_off"]) + R]
            assert not A[Rn:].any() and not A1[Rn:].any(), where
            assert (A[:Rn] != 0).all(), where
            if not t["flags"] & CONST:
                assert (np.abs(A1[:Rn] - A[:Rn]) >= F32(0.2) * np.abs(A[:Rn])).all(), where
            b = bound(int(cls), t)
            for k, v in c.mut[i].items():
                assert v >= 10 * b, (where, k, v, b)
            assert ("t" in c.mut[i]) == (not t["flags"] & CONST)
        for j in c.jobs:
            A = np.abs(c.amps[int(j["a_off"]):int(j["a_off"]) + int(j["Rn"])].astype(np.float64))
            r = np.arange(1, len(A) + 1, dtype=np.float64)
            assert (2 * np.pi) ** 4 * (A * r ** 4).sum() / (384.0 * 2.0 ** (4 * int(j["logn"]))) <= TAB_TOL * A.sum()


# ---- GPU -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    from soundgen_beta_amd import native
    c = native.Context(0)
    yield c
    c.close()


def hook(ctx, tasks, amps, wlen, jobs=None, env=ENV_VALUE, fill=None):
    """sg_debug_sine_bank: (code, W, W64, taskmax, cls); the outputs start as `fill`."""
    from soundgen_beta_amd import native
    tasks = np.ascontiguousarray(tasks, TASK)
    amps = np.ascontiguousarray(amps, F32)
    jobs = np.zeros(0, JOB) if jobs is None else np.ascontiguousarray(jobs, JOB)
    W = np.full(wlen, np.nan if fill is None else fill, F32)
    W64 = np.full(wlen, np.nan if fill is None else fill, np.float64)
    tm = np.full(len(tasks), np.nan if fill is None else fill, F32)
    cls = np.full(len(tasks), -1, np.int32)
    fp = C.POINTER(C.c_float)
    rc = native.lib().sg_debug_sine_bank(
        ctx.ptr, tasks.ctypes.data, len(tasks), amps.ctypes.data_as(fp), len(amps), wlen,
        jobs.ctypes.data if len(jobs) else None, len(jobs), env, W.ctypes.data_as(fp),
        W64.ctypes.data_as(C.POINTER(C.c_double)), tm.ctypes.data_as(fp), cls.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, W, W64, tm, cls


def check_case(ctx, name):
    from soundgen_beta_amd import native
    c = case(name)
    rc, W, W64, tm, cls = hook(ctx, c.tasks, c.amps, c.wlen, c.jobs)
    native.check(rc, ctx.ptr)
    assert (cls == c.want).all(), (name, np.flatnonzero(cls != c.want)[:8])
    hp = name == "hp"
    out = W64 if hp else W
    covered = np.zeros(c.wlen, bool)
    worst = {}
    y32 = []
    for i, t in enumerate(c.tasks):
        o, n = int(t["w_off"]) + int(t["j0"]), int(t["len"])
        assert not covered[o:o + n].any()
        covered[o:o + n] = True
        got = out[o:o + n]
        dev = np.abs(got.astype(LD) - c.ref[i]) / c.norm[i]
        k = bound_key(int(c.want[i]), t)
        worst[k] = max(worst.get(k, (0.0, -1)), (float(dev.max()), i))
        b = bound(int(c.want[i]), t)
        assert (dev <= b).all(), (name, i, int(np.argmax(~(dev <= b))), float(np.nanmax(dev)), b, t)
        y32.append(got.astype(F32))
    for k, (v, i) in sorted(worst.items(), key=str):
        t = c.tasks[i]
        print("case %-10s class %-10s %-5s GPU %.3g  restatement %.3g  bound %.3g  (worst: task %d, len %d, Rn %d, "
              "flags %d, %.0f Hz)" % (name, CLASS_NAMES[k[0]], k[1], v, measured()[k],
                                      FACTOR * measured()[k] + (TAB_TOL if k[0] == TABLE else 0), i, t["len"], t["Rn"],
                                      t["flags"], t["c1"] * SR))
    # nothing outside the tasks, nothing at all in the other precision
    assert (out.view(np.uint64 if hp else np.uint32)[~covered] == (2 ** 64 - 1 if hp else 2 ** 32 - 1)).all(), name
    other = W.view(np.uint32) if hp else W64.view(np.uint64)
    assert (other == (2 ** 32 - 1 if hp else 2 ** 64 - 1)).all(), name
    # maxima, exactly: from the samples the hook itself returned
    def window(i):
        t = c.tasks[i]
        j = int(t["j0"]) + np.arange(int(t["len"]))
        v = y32[i][(j >= t["dj0"]) & (j < t["dj1"])]
        return (v.astype(np.float64) * ENV_VALUE).astype(F32) if t["flags"] & ENV else v
    runs = []
    for i, t in enumerate(c.tasks):
        if c.want[i] in (PAIRS, TALL_PAIRS):
            prev = runs[-1] if runs else None
            if prev and c.want[prev[0]] == c.want[i] and c.tasks[prev[0]]["syl"] == t["syl"] and len(prev) < RUN_TASKS:
                prev.append(i)
            else:
                runs.append([i])
        else:  # one slot per task: the larger of 0 and its window's samples
            assert tm[i] == max(F32(0), window(i).max(initial=F32(0))), (name, i, tm[i])
    for r in runs:  # a lane outside the window or past len contributes 0; the run's max to its first slot
        want = max(max(window(i).max(initial=-np.inf), 0.0 if len(window(i)) < 64 else -np.inf) for i in r)
        assert tm[r[0]] == F32(want), (name, r, tm[r[0]], want)
        assert all(tm[i] == -np.inf for i in r[1:]), (name, r)
    for s in np.unique(c.tasks["syl"]):
        idx = np.flatnonzero(c.tasks["syl"] == s)
        samples = max(window(i).max(initial=F32(0)) for i in idx)
        assert max(F32(0), tm[idx].max()) == max(F32(0), samples), (name, int(s))


@pytest.mark.gpu
def test_long(ctx):
    """sg_sine_bank: CONST, two-column and enveloped tasks in one call.
    MI355X: largest normalised deviation 1.31e-05 against the bound 1.84e-05 (restatement 2.30e-06)."""
    check_case(ctx, "long")


@pytest.mark.gpu
def test_pairs(ctx):
    """sg_sine_bank_pairs.
    MI355X: 8.0e-07 against the bound 3.04e-06 (restatement 3.80e-07)."""
    check_case(ctx, "pairs")


@pytest.mark.gpu
def test_tall(ctx):
    """sg_sine_bank_tall.
    MI355X: 1.05e-07 against the bound 1.12e-06 (restatement 1.40e-07)."""
    check_case(ctx, "tall")


@pytest.mark.gpu
def test_tall_pairs(ctx):
    """sg_sine_bank_tall_pairs.
    MI355X: 8.64e-07 against the bound 9.18e-06 (restatement 1.15e-06)."""
    check_case(ctx, "tall_pairs")


@pytest.mark.gpu
def test_hp(ctx):
    """sg_sine_bank_hp: the samples in W64, the fp32 scratch untouched.
    MI355X: two-column tasks 8.45e-08 against 6.98e-07 (restatement 8.72e-08), CONST tasks 2.78e-11
    against 2.00e-10 (restatement 2.49e-11)."""
    check_case(ctx, "hp")


@pytest.mark.gpu
def test_table(ctx):
    """sg_sine_bank_tab in W mode, and the two tasks no job covers on sg_sine_bank.
    MI355X: table tasks 2.39e-07 against the bound 1.51e-06 (restatement 1.76e-07, SG_TAB_TOL 1e-07);
    the two recurrence tasks 2.82e-07 against the long class's 1.84e-05."""
    check_case(ctx, "table")


def _valid(n=3):
    """n valid CONST | LIN tasks on one column of 16 rows, for 40 floats of amplitudes and a scratch of 2000."""
    t = np.zeros(n, TASK)
    for i in range(n):
        t[i]["w_off"], t[i]["len"], t[i]["R"], t[i]["Rn"] = 100 * i, 70, 16, 8
        t[i]["a_off"], t[i]["d_off"], t[i]["c1"], t[i]["invD"] = 4, 20, 0.01, 1.0
        t[i]["dj1"], t[i]["flags"], t[i]["syl"] = 70, CONST | LIN, 0
    return t


def _job(**kw):
    j = np.zeros(1, JOB)
    j[0]["a_off"], j[0]["Rn"], j[0]["n"], j[0]["logn"] = 4, 8, 3, 8
    for k, v in kw.items():
        j[0][k] = v
    return j


REFUSAL_WLEN = 2000


@functools.lru_cache(maxsize=None)
def refusals():
    """(rule, tasks, jobs or None, the complaint of sine_bank_args_check): one record, or one
    set of records, per rule of the hook's validation, each breaking that rule alone."""
    def one(**kw):
        t = _valid(1)
        for k, v in kw.items():
            t[0][k] = v
        return t
    out = [("len 0", one(len=0), "len outside"),
           ("len over SG_TASK_MAX", one(len=TASK_MAX + 1), "len outside"),
           ("R 0", one(R=0), "R not a positive multiple"),
           ("R not a multiple of 16", one(R=24), "R not a positive multiple"),
           ("Rn 0", one(Rn=0), "Rn not a multiple"),
           ("Rn over R", one(Rn=20), "Rn not a multiple"),
           ("Rn not a multiple of 4", one(Rn=6), "Rn not a multiple"),
           ("j0 negative", one(j0=-1, w_off=1), "j0 negative"),
           ("mbase negative", one(mbase=-1), "mbase outside"),
           ("before the scratch", one(j0=3, w_off=-4), "samples outside the scratch"),
           ("past the scratch", one(w_off=REFUSAL_WLEN - 69), "samples outside the scratch"),
           ("w_off near the end of int64", one(w_off=2 ** 63 - 1, j0=2 ** 31 - 1), "samples outside the scratch"),
           ("a_off negative", one(a_off=-1), "a_off outside"),
           ("a_off + R past the amplitudes", one(a_off=25), "a_off outside"),
           ("a_off near the end of int64", one(a_off=2 ** 63 - 1), "a_off outside"),
           ("d_off negative", one(flags=0, d_off=-16), "d_off outside"),
           ("d_off + R past the amplitudes", one(flags=0, d_off=25), "d_off outside"),
           ("dj0 negative", one(dj0=-1), "window not"),
           ("dj0 over dj1", one(dj0=71), "window not"),
           ("syl negative", one(syl=-1), "syl negative"),
           ("unknown flag", one(flags=16 | CONST), "unknown flag"),
           ("ENV with LIN", one(flags=ENV | LIN), "SG_TASK_ENV with SG_TASK_LIN"),
           ("c1 not finite", one(c1=np.inf), "coefficient not finite")]
    out = [(n, t, None, w) for n, t, w in out]
    t = _valid(3)
    t["syl"] = (5, 6, 5)
    out.append(("a syllable's tasks apart", t, None, "tasks of one syllable apart"))
    t = _valid(3)
    out += [("n 0", t, _job(n=0), "job n outside"),
            ("n over SG_TAB_TASKS", np.repeat(_valid(1), 65), _job(n=65), "job n outside"),
            ("t0 + n past the tasks", t, _job(t0=1), "job tasks out of range"),
            ("t0 negative", t, _job(t0=-1, n=1), "job tasks out of range"),
            ("two jobs on one task", t, np.concatenate([_job(n=2), _job(t0=1, n=2)]), "job tasks out of range"),
            ("logn under SG_TAB_LOGN_MIN", t, _job(logn=7), "job logn"),
            ("logn over SG_TAB_LOGN_MAX", t, _job(logn=12), "job logn"),
            ("job flags", t, _job(flags=1), "job flags"),
            ("job a_off past the amplitudes", t, _job(a_off=33), "job a_off outside")]
    u = _valid(3)
    u["Rn"] = 4
    out.append(("Rn under 4", u, _job(Rn=0), "job Rn outside"))
    u = _valid(3)
    u["R"], u["Rn"], u["a_off"], u["d_off"] = 112, 100, 0, 0
    out.append(("Rn over SG_ROWS_F32", u, _job(Rn=100, a_off=0), "job Rn outside"))
    for name, f in (("covered task not LIN", CONST), ("covered task not CONST", LIN),
                    ("covered task HP", CONST | LIN | HP)):
        u = _valid(3)
        u[1]["flags"] = f
        out.append((name, u, _job(), "job task not"))
    u = _valid(3)
    u[2]["a_off"] = 0
    out.append(("covered task on another column", u, _job(), "job task not"))
    u = _valid(3)
    u[2]["Rn"] = 4
    out.append(("covered task with another Rn", u, _job(), "job task not"))
    return out


def refusal_amps(t):
    return np.zeros(112 if t["R"].max() > 16 else 40, F32)


@pytest.mark.parametrize("flags", [("-O2",), ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")],
                         ids=["plain", "sanitized"])
def test_validation_on_the_host(tmp_path, flags):
    """sine_bank_args_check alone (a stand-alone program, run directly), plain and under the
    address and undefined-behaviour sanitizers: every case of this file passes, every record
    of refusals() is refused with the complaint of the rule it breaks, and so are an empty
    call, a scratch or an amplitude array of no elements and an envelope that is not finite."""
    exe = str(tmp_path / "sine_bank_check")
    subprocess.run(["g++", "-std=c++17", *flags, "-I" + CSRC, os.path.join(HERE, "cpp", "sine_bank_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    cases = [(name, case(name).tasks, len(case(name).amps), case(name).wlen, case(name).jobs, ENV_VALUE, "ok")
             for name in BUILDERS]
    cases += [(n, t, len(refusal_amps(t)), REFUSAL_WLEN, np.zeros(0, JOB) if j is None else j, 1.0, w)
              for n, t, j, w in refusals()]
    v = _valid(1)
    cases += [("valid", v, 40, REFUSAL_WLEN, np.zeros(0, JOB), 1.0, "ok"),
              ("valid with a job", _valid(3), 40, REFUSAL_WLEN, _job(), 1.0, "ok"),
              ("no tasks", v[:0], 40, REFUSAL_WLEN, np.zeros(0, JOB), 1.0, "ntasks out of range"),
              ("no scratch", v, 40, 0, np.zeros(0, JOB), 1.0, "wlen out of range"),
              ("no amplitudes", v, 0, REFUSAL_WLEN, np.zeros(0, JOB), 1.0, "namps out of range"),
              ("more jobs than tasks", v, 40, REFUSAL_WLEN, np.repeat(_job(n=1), 2), 1.0, "njobs out of range"),
              ("env not finite", v, 40, REFUSAL_WLEN, np.zeros(0, JOB), float("nan"), "env not finite")]
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(np.int64(len(cases)).tobytes())
        for _, t, namps, wlen, j, env, _ in cases:
            f.write(np.array([len(t), namps, wlen, len(j)], np.int64).tobytes())
            f.write(np.float64(env).tobytes())
            f.write(np.ascontiguousarray(t, TASK).tobytes())
            f.write(np.ascontiguousarray(j, JOB).tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = r.stdout.splitlines()
    assert len(got) == len(cases)
    for (name, *_, want), line in zip(cases, got):
        assert line.startswith(want), (name, line, want)


@pytest.mark.gpu
def test_refusals(ctx):
    """One invalid record (or set) per rule of the hook's validation: SG_E_ARG with the rule's
    complaint as the context's error text, and the outputs keep what the caller put there.
    Every call here is refused, so nothing is launched."""
    from soundgen_beta_amd import native
    assert len(refusals()) >= 35
    for name, t, j, why in refusals():
        rc, W, W64, tm, cls = hook(ctx, t, refusal_amps(t), REFUSAL_WLEN, j, fill=-7.25)
        assert rc == -1, name
        assert why in native.lib().sg_last_error(ctx.ptr).decode(), name
        assert (W == -7.25).all() and (W64 == -7.25).all() and (tm == -7.25).all() and (cls == -1).all(), name
    assert hook(ctx, _valid(1), refusal_amps(_valid(1)), REFUSAL_WLEN, env=float("nan"), fill=-7.25)[0] == -1
