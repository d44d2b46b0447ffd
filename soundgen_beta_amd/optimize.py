"""optimizePars() and segmentFolder() (R/optimize.R:110-234, R/segment.R:254-304) on the GPU.

optimizePars evaluates segmentFolder() or analyzeFolder() many times on the same sounds
while only a few parameters change. Here the files are read and uploaded once, and for
segmentFolder a set of parameter vectors is one sweep (sg_segment_sweep, sg_segment.hip):
the raw Hilbert envelope once per sound, the smoothed one once per sound and
(windowLength, overlap), the tail of all (sound, vector) pairs in one launch, the summaries
left in HBM; the default fitness (1 - Pearson correlation with the key over the complete
pairs) is computed there too (sg_sweep_fitness). For analyzeFolder a set of vectors is one
sweep per sampling rate likewise (analyze.analyze_sweep, sg_analyze_sweep in sg_analyze.hip):
the spectrogram and the amplitudes once per distinct window and step, the autocorrelations
once per distinct gates and lag band, the candidates once per distinct set of the per-frame
decisions, and the pathfinder, the harmonics and the summary of all (sound, vector) pairs in
one launch each. Only a vector whose otherPars ask for the formant columns is still one
analyze_batch(summary=True).

A vector's summaries and fitness do not depend on the vectors it shares a sweep with (the
same bits), so the Nelder-Mead restarts can evaluate their candidates ahead of time and
together without changing any trajectory (nelder_mead).

Quirks of the reference that are kept:
  * without `init` the starting values are the function's defaults of the names in `pars`
    in the order of the function's FORMALS (optimize.R:152), while evaluatePars names the
    values by `pars` (:221-222): a `pars` given in another order than the formals pairs
    values and names wrongly, here as there;
  * evaluatePars' bounds rule: a vector outside `bounds` scores 1 and is not evaluated
    (:217-220); with `mygrid` evaluatePars gets no bounds and every row is evaluated;
  * the result's rows are ordered by r decreasing with order(): stable, NaN last.
Stated differences: a parameter whose default is NULL (interburst, step, ...) makes
unlist() drop it in R and the optimizer then runs on a shorter vector; that raises
ValueError here. verbose prints one line per evaluated vector, also for the candidates
evaluated ahead of time. The simplex is restated from the documented algorithm of R's
nmmin (see nelder_mead); its trajectory is not pinned against R. Plots and the progress
reports are out of scope.
"""
import ctypes as C
import inspect
import math

import numpy as np

from . import native
from . import segment as SG

GRID_NAMES = ("windowLength", "overlap", "shortestSyl", "shortestPause", "sylThres", "interburst", "interburstMult",
              "burstThres", "peakToTrough")
# segmentFolder's formals in their order (segment.R:254-271) with their defaults; None is NULL
SEGMENT_FOLDER_FORMALS = (("shortestSyl", 40), ("shortestPause", 40), ("sylThres", 0.9), ("interburst", None),
                          ("interburstMult", 1), ("burstThres", 0.075), ("peakToTrough", 3), ("troughLeft", True),
                          ("troughRight", False), ("windowLength", 40), ("overlap", 80), ("summary", True),
                          ("plot", False), ("savePath", math.nan), ("verbose", True), ("reportEvery", 10))
_SEGMENT_SET = GRID_NAMES + ("troughLeft", "troughRight")
_GRID_ERROR = "mygrid should be either NULL or a dataframe with one column per parameter"
_BIG = 1.0e35


# ------------------------------------------------------------------------ the sweep
def _null(v):
    return v is None or (isinstance(v, (float, np.floating)) and math.isnan(v))


def _sweep(data, offsets, lengths, samplingRate, rows, workspace_cap=0, device=0):
    """sg_segment_sweep over `rows`, dicts of segment()'s arguments (absent: its defaults):
    the fp64 CUDA tensor of shape (rows, sounds, 11)."""
    from . import _abi
    offs, lens, nc, p_offs, p_lens = native.batch_layout(offsets, lengths)
    P = (_abi.sg_segment_params * max(len(rows), 1))()
    for r, kw in enumerate(rows):
        kw = dict(kw)
        for k in ("shortestPause", "interburst"):
            if k in kw and _null(kw[k]):
                kw[k] = None
        ib = kw.get("interburst")
        if ib is not None and (isinstance(ib, bool) or not isinstance(ib, (int, float, np.integer, np.floating)) or ib < 0):
            raise ValueError("interburst is weird or negative: %r" % (ib,))
        if "overlap" in kw:
            kw["overlap"] = min(max(kw["overlap"], 0), 99)
        P[r] = SG._params(samplingRate, mode=0, workspace_cap=workspace_cap, **kw)
    ctx = native.default_context(device)
    out = native.device_out(data, len(rows) * nc * 11)
    SG._check(native.lib().sg_segment_sweep(ctx.ptr, C.c_void_p(data.data_ptr()), p_offs, p_lens, nc, P, len(rows),
                                            C.c_void_p(out.data_ptr())), ctx.ptr)
    return out[:len(rows) * nc * 11].reshape(len(rows), nc, 11)


def segment_sweep(data, offsets, lengths, samplingRate, grid, troughLeft=True, troughRight=False, to_host=True,
                  workspace_cap=0, device=0):
    """segment(call i, samplingRate, summary = TRUE) under every row of a parameter grid for
    a batch of sounds already in HBM (the layout of segment_batch()), as one launch
    sequence (sg_segment_sweep). grid: a dict from any of GRID_NAMES to equally long
    sequences, one entry per row; absent names take segment()'s defaults; None or NaN in
    shortestPause / interburst mean NULL. Returns the array of shape (rows, sounds, 11),
    the cells named by segment.SUMMARY_COLUMNS (NaN for NA), or the fp64 CUDA tensor for
    to_host=False. Row g of sound i equals segment_batch(summary=True) under row g's
    parameters bit for bit, whatever the other rows and whatever workspace_cap (bytes of
    transform workspace per chunk of sounds and of tables per chunk of rows; 0: the
    library's default). A sound the reference stops on (fewer than three samples) has nSyl
    = nBursts = 0 and NaN elsewhere. A row the planner refuses for any sound refuses the
    sweep before anything is launched."""
    bad = [k for k in grid if k not in GRID_NAMES]
    if bad:
        raise ValueError("segment_sweep: not a parameter of the grid: %s" % ", ".join(bad))
    cols = {k: list(v) for k, v in grid.items()}
    n = {len(v) for v in cols.values()}
    if len(n) > 1:
        raise ValueError("segment_sweep: the grid's columns differ in length")
    n = n.pop() if n else 0
    rows = [dict({k: v[r] for k, v in cols.items()}, troughLeft=troughLeft, troughRight=troughRight) for r in range(n)]
    out = _sweep(data, offsets, lengths, samplingRate, rows, workspace_cap, device)
    return out.cpu().numpy() if to_host else out


def sweep_fitness(matrix, column, key, device=0):
    """1 - cor(x, key, use = 'pairwise.complete.obs'), optimizePars' default fitnessFun, for
    every row of `matrix` on the GPU (sg_sweep_fitness): matrix is an fp64 CUDA tensor of
    shape (rows, sounds, width) or (sounds, width) -- segment_sweep(to_host=False)'s, or
    analyze_batch(summary=True)['out'] --, x its column `column` (an index, or a name of
    segment.SUMMARY_COLUMNS for width 11 and of analyze.SUMMARY_COLUMNS for width 44), key
    one number per sound; NaN is NA on either side and drops the pair. Returns one float per
    row: NaN for fewer than two complete pairs or a side whose values are all equal."""
    import torch
    if matrix.dim() == 2:
        matrix = matrix.unsqueeze(0)
    if matrix.dim() != 3 or matrix.dtype != torch.float64 or not matrix.is_cuda:
        raise ValueError("sweep_fitness: matrix must be an fp64 CUDA tensor of shape (rows, sounds, width)")
    matrix = matrix.contiguous()
    rows, nc, width = matrix.shape
    if isinstance(column, str):
        column = _column(column, width)
    key = np.ascontiguousarray(np.asarray(key, dtype=np.float64).ravel())
    if len(key) != nc:
        raise ValueError("sweep_fitness: the key has %d values for %d sounds" % (len(key), nc))
    fit = np.zeros(rows)
    ctx = native.default_context(device)
    torch.cuda.synchronize(matrix.device)  # the library runs on its own stream
    dp = C.POINTER(C.c_double)
    SG._check(native.lib().sg_sweep_fitness(ctx.ptr, C.c_void_p(matrix.data_ptr()), rows, nc, width, int(column),
                                            key.ctypes.data_as(dp), fit.ctypes.data_as(dp)), ctx.ptr)
    return fit


def _column(name, width):
    from . import analyze as AN
    names = {11: SG.SUMMARY_COLUMNS, 44: AN.SUMMARY_COLUMNS}.get(width)
    if names is None or name not in names:
        raise ValueError("no column %r in a summary of %d cells" % (name, width))
    return names.index(name)


# ------------------------------------------------------------------- segmentFolder()
def _stopped_row():
    r = dict.fromkeys(SG.SUMMARY_COLUMNS, math.nan)
    r["nSyl"] = r["nBursts"] = 0
    return r


def segment_folder(myfolder, shortestSyl=40, shortestPause=40, sylThres=0.9, interburst=None, interburstMult=1,
                   burstThres=0.075, peakToTrough=3, troughLeft=True, troughRight=False, windowLength=40, overlap=80,
                   summary=True, plot=False, savePath=None, verbose=True, reportEvery=10, device=0):
    """segmentFolder() (R/segment.R:254-304) on the GPU: segment() for every .wav file of
    myfolder. The files are listed, read, grouped by sampling rate and uploaded as
    analyze_folder() does (analyze.folder_groups); each group is one segment_batch().

    summary=True: a list of dicts in file order, `sound` (the base name) first, then the
    eleven cells of segment.SUMMARY_COLUMNS; a row equals segment_batch(summary=True) of
    the file's samples bit for bit. A file of fewer than three samples, on which segment()
    stops, has nSyl = nBursts = 0 and NaN elsewhere. summary=False: a dict from the file's
    full path to its segment() value (None for such a file). plot=True and a savePath
    raise before any file is read; verbose and reportEvery are accepted and print nothing."""
    from . import analyze as AN
    if plot or isinstance(savePath, str):
        raise NotImplementedError("segment_folder(plot = TRUE / savePath): plotting is out of scope")
    names, paths, groups = AN.folder_groups(myfolder, device)
    results = [None] * len(paths)
    for g in groups:
        got = SG.segment_batch(g["data"], g["offsets"], g["lengths"], g["samplingRate"], windowLength, overlap,
                               shortestSyl, shortestPause, sylThres, interburst, interburstMult, burstThres, peakToTrough,
                               troughLeft, troughRight, summary=bool(summary), device=device)
        for i, r in zip(g["files"], got):
            results[i] = r
    if summary:
        return [dict([("sound", n)] + list((_stopped_row() if r is None else r).items())) for n, r in zip(names, results)]
    return dict(zip(paths, results))


# ----------------------------------------------------------------------- Nelder-Mead
def _nm_steps(par, maxit, reltol, abstol, alpha, beta, gamma, trace):
    """The sequential algorithm as a generator: yields (x, ahead) -- x the vector whose value
    it needs now, `ahead` the vectors it may ask for next, known already -- and receives x's
    value. Returns dict(par, value, counts, convergence)."""
    n = len(par)
    b = [float(v) for v in par]

    def note(kind, x, f):
        if trace is not None:
            trace(kind, list(x), f)

    def value(f):
        return f if math.isfinite(f) else _BIG

    step = max([0.1 * abs(v) for v in b] + [0.0])
    if step == 0.0:
        step = 0.1
    P = [list(b)]  # the vertices; F their values
    size = 0.0
    for j in range(1, n + 1):
        v = list(b)
        trystep = step
        while v[j - 1] == b[j - 1]:
            v[j - 1] = b[j - 1] + trystep
            trystep *= 10
        size += trystep
        P.append(v)
    f = yield list(b), [list(v) for v in P[1:]]
    note("eval", b, f)
    if maxit <= 0:
        return dict(par=b, value=f, counts=0, convergence=0)
    if not math.isfinite(f):
        raise ValueError("function cannot be evaluated at initial parameters")
    count = 1
    convtol = reltol * (abs(f) + reltol)
    F = [f] + [None] * n
    L, oldsize, calcvert, fail = 0, size, True, 0
    while True:
        if calcvert:
            todo = [j for j in range(n + 1) if j != L]
            for k, j in enumerate(todo):
                f = yield list(P[j]), [list(P[i]) for i in todo[k + 1:]]
                note("eval", P[j], f)
                F[j] = value(f)
                count += 1
            calcvert = False
        VL = VH = F[L]
        H = L
        L0 = L
        for j in range(n + 1):
            if j != L0:
                if F[j] < VL:
                    L, VL = j, F[j]
                if F[j] > VH:
                    H, VH = j, F[j]
        if VH <= VL + convtol or VL <= abstol:
            break
        cen = [(sum(P[j][i] for j in range(n + 1)) - P[H][i]) / n for i in range(n)]
        R = [(1.0 + alpha) * cen[i] - alpha * P[H][i] for i in range(n)]
        E = [gamma * R[i] + (1 - gamma) * cen[i] for i in range(n)]
        KH = [(1 - beta) * P[H][i] + beta * cen[i] for i in range(n)]
        KR = [(1 - beta) * R[i] + beta * cen[i] for i in range(n)]
        f = yield list(R), [E, KH, KR]
        note("eval", R, f)
        VR = value(f)
        count += 1
        if VR < VL:
            f = yield list(E), []
            note("eval", E, f)
            f = value(f)
            count += 1
            if f < VR:
                P[H], F[H] = E, f
                note("EXTENSION", E, f)
            else:
                P[H], F[H] = R, VR
                note("REFLECTION", R, VR)
        else:
            action = "HI-REDUCTION"
            K = KH
            if VR < VH:
                P[H], F[H] = R, VR
                action, K = "LO-REDUCTION", KR
            f = yield list(K), []
            note("eval", K, f)
            f = value(f)
            count += 1
            if f < F[H]:
                P[H], F[H] = K, f
                note(action, K, f)
            elif VR >= VH:
                calcvert = True
                size = 0.0
                for j in range(n + 1):
                    if j != L:
                        for i in range(n):
                            P[j][i] = beta * (P[j][i] - P[L][i]) + P[L][i]
                            size += abs(P[j][i] - P[L][i])
                note("SHRINK", P[L], F[L])
                if size < oldsize:
                    oldsize = size
                else:
                    fail = 10
                    break
        if not count <= maxit:
            break
    if count > maxit:
        fail = 1
    return dict(par=list(P[L]), value=F[L], counts=count, convergence=fail)


class _Simplex:
    """One run of _nm_steps with the values it was given ahead of time."""

    def __init__(self, par, speculate, **kw):
        self.gen = _nm_steps(par, **kw)
        self.speculate = speculate
        self.known = {}
        self.result = None
        self.want = None
        self._next(None)

    def _next(self, value):
        try:
            self.want = self.gen.send(value)
        except StopIteration as e:
            self.result, self.want = e.value, None

    def pending(self):
        """The vectors to evaluate now ([] when finished): the one the algorithm waits for,
        then those it may ask for next. Values known already are consumed first."""
        while self.want is not None and tuple(self.want[0]) in self.known:
            self._next(self.known[tuple(self.want[0])])
        if self.want is None:
            return []
        return [self.want[0]] + (self.want[1] if self.speculate else [])

    def feed(self, vectors, values):
        self.known = {tuple(x): float(v) for x, v in zip(vectors, values)}


def nelder_mead_many(fn_many, starts, maxit=500, reltol=math.sqrt(2.220446049250313e-16), abstol=-math.inf, alpha=1.0,
                     beta=0.5, gamma=2.0, speculate=True, trace=None):
    """nelder_mead() from every vector of `starts`, in lockstep: each round is one call of
    fn_many with what all unfinished runs need (and, with speculate, may need next). Every
    run is the sequential algorithm's, whatever the others do. trace(kind, x, f), if given,
    gets one more leading argument, the run's index. Returns the list of results."""
    kw = dict(maxit=maxit, reltol=reltol, abstol=abstol, alpha=alpha, beta=beta, gamma=gamma)
    runs = [_Simplex(p, speculate, trace=None if trace is None else (lambda k, x, f, i=i: trace(i, k, x, f)), **kw)
            for i, p in enumerate(starts)]
    while True:
        asks = [(s, s.pending()) for s in runs]
        asks = [(s, v) for s, v in asks if v]
        if not asks:
            return [s.result for s in runs]
        values = list(fn_many([x for _, v in asks for x in v]))
        at = 0
        for s, v in asks:
            s.feed(v, values[at:at + len(v)])
            at += len(v)


def nelder_mead(fn_many, par, maxit=500, reltol=math.sqrt(2.220446049250313e-16), abstol=-math.inf, alpha=1.0, beta=0.5,
                gamma=2.0, speculate=True, trace=None):
    """optim(method = 'Nelder-Mead'): R's nmmin, minimizing from `par`. fn_many takes a list of
    vectors and returns their values. Returns dict(par, value, counts, convergence: 0, 1
    when maxit was reached, 10 for a degenerate simplex).

    R's C sources were not at hand: this restates the documented algorithm with optim()'s
    constants (alpha = 1, beta = 0.5, gamma = 2, reltol = sqrt(.Machine$double.eps), maxit =
    500), and the trajectory is not pinned against R. What is followed:
      * the initial step is 0.1 x the largest |par_i|, or 0.1 when all are zero; vertex j
        moves coordinate j - 1 by it, and by 10 x as much while the sum does not change the
        coordinate;
      * a value that is not finite counts as 1e35; at the start it is an error;
      * convtol = reltol (|f0| + reltol); stop when f_high <= f_low + convtol or f_low <=
        abstol;
      * the centroid C is over all vertices but the worst, H; the reflection R = (1 + alpha)
        C - alpha H;
      * f_R < f_low: the expansion E = gamma R + (1 - gamma) C; the better of R and E
        replaces H;
      * otherwise, if f_R < f_high, R replaces H first; the contraction is (1 - beta) H + beta
        C with that H, accepted when below the current f_high; if it is not and f_R >= f_high,
        every vertex moves halfway (beta) to the best one and all are evaluated again; the run
        fails (10) when the sum of their distances to the best did not decrease;
      * every evaluation counts, and the loop runs while the count is <= maxit.
    The candidates of a step -- R, E, (H + C) / 2 and (R + C) / 2 -- are known before any
    is evaluated. With speculate they go to fn_many together with R, and the algorithm then
    consumes the values it needs: the vertices, the values and the count that maxit limits
    are those of the sequential algorithm (fn_many must give a vector the same value
    whatever it is evaluated with). trace(kind, x, f): 'eval' for every evaluation the
    sequential algorithm makes, and 'REFLECTION', 'EXTENSION', 'HI-REDUCTION', 'LO-REDUCTION'
    (the vertex that replaced the worst) and 'SHRINK'."""
    t = None if trace is None else (lambda i, k, x, f: trace(k, x, f))
    return nelder_mead_many(fn_many, [par], maxit, reltol, abstol, alpha, beta, gamma, speculate, t)[0]


# --------------------------------------------------------------------- optimizePars()
def _formals(myfun):
    from . import analyze as AN
    if myfun == "segmentFolder":
        return SEGMENT_FOLDER_FORMALS
    if myfun == "analyzeFolder":
        sig = inspect.signature(AN.analyze_folder).parameters
        return tuple((k, v.default) for k, v in sig.items() if k not in ("myfolder", "device"))
    raise ValueError("myfun must be 'segmentFolder' or 'analyzeFolder'")


def start_means(myfun, pars, init=None):
    """as.numeric(unlist(pars_defaults)) (optimize.R:151-164): `init` as given, or the
    defaults of the names in `pars` in the order of the function's formals."""
    if init is not None:
        vals = list(init.values()) if isinstance(init, dict) else list(np.atleast_1d(init))
        return [float(v) for v in vals]
    formals = _formals(myfun)
    out = []
    for name, default in formals:
        if name not in pars:
            continue
        if default is None:
            raise ValueError("optimize_pars: the default of %s is NULL, which unlist() drops in the reference; give init"
                             % name)
        if isinstance(default, (str, tuple, list, dict)) or (isinstance(default, float) and math.isnan(default)):
            raise ValueError("optimize_pars: the default of %s is not a number; give init" % name)
        out.append(float(default))
    return out


def draw_starts(means, initSD, low, high, nIter, rng):
    """p_init of every iteration (optimize.R:161-166), drawn from rng in R's order."""
    from .matchpars import _Draws, rnorm_bounded
    D = _Draws(rng)
    return [rnorm_bounded(D, len(means), means, [m * initSD for m in means], low, high) for _ in range(int(nIter))]


def name_values(pars, p):
    """params = as.list(p); names(params) = pars (optimize.R:221-222): by position."""
    return {k: float(v) for k, v in zip(pars, p)}


def order_decreasing(r):
    """order(r, decreasing = TRUE): stable, NaN last."""
    r = [float(v) for v in r]
    ok = [i for i in range(len(r)) if not math.isnan(r[i])]
    return sorted(ok, key=lambda i: -r[i]) + [i for i in range(len(r)) if math.isnan(r[i])]


def bounded(evaluate, low, high):
    """evaluatePars' bounds rule (optimize.R:217-220) around evaluate(list of vectors): a
    vector with a value below `low` or above `high` scores 1 and is not evaluated."""
    low, high = np.asarray(low, float), np.asarray(high, float)

    def fn_many(vectors):
        inside = [i for i, p in enumerate(vectors) if not (np.any(np.asarray(p) < low) or np.any(np.asarray(p) > high))]
        out = [1.0] * len(vectors)
        if inside:
            for i, v in zip(inside, evaluate([vectors[i] for i in inside])):
                out[i] = float(v)
        return out
    return fn_many


class _Folder:
    """The sounds of a folder in HBM and what optimizePars evaluates on them."""

    def __init__(self, myfolder, key, myfun, pars, fitnessPar, fitnessFun, otherPars, verbose, device):
        from . import analyze as AN
        self.formals = dict(_formals(myfun))
        self.myfun, self.pars, self.fitnessFun, self.verbose, self.device = myfun, list(pars), fitnessFun, verbose, device
        other = dict(otherPars or {})
        unknown = [k for k in list(other) + self.pars if k not in self.formals]
        if unknown:
            raise ValueError("unused argument of %s: %s" % (myfun, ", ".join(unknown)))
        if other.get("plot") or isinstance(other.get("savePath"), str):
            raise NotImplementedError("optimize_pars: plotting is out of scope")
        if not other.get("summary", True):
            raise ValueError("optimize_pars needs summary = TRUE: the fitness is read from a summary column")
        if myfun == "segmentFolder":
            self.settable, self.columns = _SEGMENT_SET, SG.SUMMARY_COLUMNS
        else:
            self.settable = tuple(inspect.signature(AN.analyze_batch).parameters)[4:]
            self.settable = tuple(k for k in self.settable if k not in ("to_host", "device", "summary", "plot"))
            self.columns = AN.SUMMARY_COLUMNS
            if other.get("pathfinding") == "slow":
                raise NotImplementedError(AN._SLOW)
        if fitnessPar not in self.columns:
            raise ValueError("fitnessPar must be a column of %s's summary: %r" % (myfun, fitnessPar))
        self.column = self.columns.index(fitnessPar)
        self.other = {k: v for k, v in other.items() if k in self.settable}
        self.names, self.paths, self.groups = AN.folder_groups(myfolder, device)
        self.key = np.asarray(key, dtype=np.float64).ravel()
        if fitnessFun is None and len(self.key) != len(self.names):
            raise ValueError("optimize_pars: the key has %d values for %d files" % (len(self.key), len(self.names)))

    def summaries(self, vectors):
        """The fp64 CUDA tensor (vectors, files, width) of the summaries, in file order."""
        import torch
        from . import analyze as AN
        rows = [dict(self.other, **{k: v for k, v in name_values(self.pars, p).items() if k in self.settable})
                for p in vectors]
        dev = "cuda:%d" % self.device
        out = torch.empty((len(rows), len(self.names), len(self.columns)), dtype=torch.float64, device=dev)
        for g in self.groups:
            where = torch.as_tensor(g["files"], dtype=torch.int64, device=dev)
            if self.myfun == "segmentFolder":
                m = _sweep(g["data"], g["offsets"], g["lengths"], g["samplingRate"], rows, device=self.device)
            else:  # one sweep; a row that asks for the formant columns runs on its own, as before
                m = torch.empty((len(rows), len(g["files"]), len(self.columns)), dtype=torch.float64, device=dev)
                swept = [r for r, kw in enumerate(rows) if not kw.get("formants")]
                if swept:
                    m[swept] = AN.analyze_sweep(g["data"], g["offsets"], g["lengths"], g["samplingRate"],
                                                [rows[r] for r in swept], device=self.device)
                for r, kw in enumerate(rows):
                    if kw.get("formants"):
                        m[r] = AN.analyze_batch(g["data"], g["offsets"], g["lengths"], g["samplingRate"], to_host=False,
                                                device=self.device, summary=True, **kw)["out"]
            out[:, where, :] = m
        return out

    def evaluate(self, vectors):
        """evaluatePars (optimize.R:221-233) for a list of vectors: their fitness values."""
        try:
            m = self.summaries(vectors)
        except (ValueError, native.SoundgenError) as e:
            raise RuntimeError("Error in myfun: %s" % e) from e
        if self.fitnessFun is None:
            fit = [float(v) for v in sweep_fitness(m, self.column, self.key, self.device)]
        else:
            x = m[:, :, self.column].cpu().numpy()
            fit = [float(self.fitnessFun(x[r].copy())) for r in range(len(vectors))]
        if self.verbose:
            for p, v in zip(vectors, fit):
                print("Tried pars %s; fit = %s" % (", ".join(str(round(float(q), 3)) for q in p), round(v, 4)))
        return fit


def optimize_pars(myfolder, key, myfun, pars, bounds=None, fitnessPar=None, fitnessFun=None, nIter=10, init=None,
                  initSD=.2, control=None, otherPars=None, mygrid=None, verbose=True, rng=None, device=0, speculate=True):
    """optimizePars() (R/optimize.R:110-193) with evaluatePars (:206-234) on the GPU.

    myfun: 'segmentFolder' or 'analyzeFolder'; pars: the names of the parameters to
    optimize; key: one number per file of myfolder (in sorted order of the names), NaN for
    NA; fitnessPar: the summary column compared with the key; fitnessFun: None for the
    reference's default, 1 - cor(x, key, use = 'pairwise.complete.obs'), computed on the GPU
    (sweep_fitness), or a callable that gets the column as a numpy array (one value per
    file) and returns a number; bounds: dict(low=[...], high=[...]) or None; otherPars:
    further arguments of the folder function (plot = TRUE raises; verbose, reportEvery and
    summary = TRUE are accepted). The files are read and uploaded once. For segmentFolder a
    set of vectors is one sweep per sampling rate, and so it is for analyzeFolder (see the
    module's text).

    mygrid (option 1): a dict of equally long columns whose first len(pars) names are pars;
    every row is evaluated (no bounds, as in the reference) and the grid comes back as a
    dict with one more column, `fit` (a numpy array).

    Otherwise (option 2) nIter runs of Nelder-Mead (nelder_mead; control: maxit, reltol,
    abstol, alpha, beta, gamma, defaults maxit = 50 and reltol = 0.01 as in the reference's
    signature) from p_init = rnorm_bounded(mean = start, sd = start x initSD, low, high)
    drawn from rng (rrng.RRng; RRng(1) when None) in R's order: neither folder function
    draws, so all starts are drawn first. The runs advance in lockstep and, with speculate,
    evaluate the candidates of a step together: up to 4 x nIter vectors per sweep; the
    trajectories are those of the sequential algorithm. Returns a list of dicts in the order
    of order(r, decreasing = TRUE): `r` = 1 - the run's best value, then one entry per name
    of pars."""
    from .rrng import RRng
    pars = [pars] if isinstance(pars, str) else list(pars)
    if mygrid is not None and list(mygrid)[:len(pars)] != pars:
        raise ValueError(_GRID_ERROR)
    means = None if mygrid is not None else start_means(myfun, pars, init)
    F = _Folder(myfolder, key, myfun, pars, fitnessPar, fitnessFun, otherPars, verbose, device)
    if mygrid is not None:                                                    # :131-148
        cols = [list(mygrid[k]) for k in pars]
        rows = [[float(c[i]) for c in cols] for i in range(len(cols[0]))] if cols else []
        out = {k: list(v) for k, v in mygrid.items()}
        out["fit"] = np.array(F.evaluate(rows) if rows else [], dtype=np.float64)
        return out
    low = [-math.inf] * len(pars) if bounds is None else list(bounds["low"])
    high = [math.inf] * len(pars) if bounds is None else list(bounds["high"])
    starts = draw_starts(means, initSD, low, high, nIter, rng if rng is not None else RRng(1))
    ctl = dict(maxit=50, reltol=0.01)
    ctl.update({k: v for k, v in (control or {}).items() if k != "trace"})
    res = nelder_mead_many(bounded(F.evaluate, low, high), starts, speculate=speculate, **ctl)
    rows = [[1 - r["value"]] + list(r["par"]) for r in res]                  # :183-185
    keys = ["r"] + pars
    return [dict(zip(keys, rows[i])) for i in order_decreasing([r[0] for r in rows])]
