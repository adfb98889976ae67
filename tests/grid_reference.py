"""A deterministic grid filter: the exact likelihood and filtering distributions of a model of latent dimension d <= 3, by
quadrature on a tensor grid.  It shares no code, no variates and no elementary function with the kernels or the oracle, and its
cost does not depend on a cloud size N: a particle filter's estimate must converge to it as N grows, whatever its variates are.

Written from the model definitions (paths relative to src/main/scala/com/github/jonnylaw/model/ of the reference):

* transitions, Sde.scala: every built-in step is a linear Gaussian map per component, x' = A x + b + N(0, q) --
  Brownian (:114-123) A = 1, b = 0, q = sigma dt; GenBrownian (:86-95) b = mu dt; OU (:139-150, phi = logistic of the stored,
  already-logistic value: :136, SdeParameters.scala:204) A = exp(-phi dt), b = mu (1 - A), q = sigma^2 (1 - exp(-2 phi dt)) / (2 phi);
  the trait's Euler-Maruyama step (:23-43) with drift a + b x and diffusion g: A = 1 + b dt, b = a dt, q = g^2 dt.
  Parameter vectors are cyclically repeated to the leaf's dimension (buildParamRepeat, :177-179).  The initial state is
  N(m0, c0) per component (c0 stored as its log).  dt = 0 is the identity.
* gamma = f(x, t), Model.scala:122-128 and :217-225: the first component of every plain leaf, the dot product of
  (cos(w a t), sin(w a t))_{a = 1..harmonics}, w = 2 pi / period, with a seasonal leaf's state; summed over the leaves.
* observation potentials of the leftmost leaf (Model.scala:118-120,132), in numpy / scipy.special with the parametrisations of
  tests/golden/make_golden.py.  A missing observation has no potential.
* the estimator convention of stepFilter (ParticleFilter.scala:116-132): ll += log of the integral of the prediction times the
  potential; the clock starts at min(t).
* LGCP, FilterLgcp (ParticleFilter.scala:184-226): nsub = ceil(dt / delta) sub-steps of delta = 10^-precision, the clock started
  at the observation's own time; each sub-step moves, advances the clock and multiplies by exp(-exp(gamma(x, tau)) delta); the
  event multiplies by exp(gamma(x, t)).  dt = 0 weighs every particle by exp(0).

The grid.  Each step's grid is a tensor product of uniform axes, each centred on the exact Gaussian envelope of the prediction
(the posterior's per-axis mean and variance pushed through the linear transition) and covering +-12 of its sd (+-10 leaves 2e-12 of a Student-t posterior outside); the spacing is
1/6 of the smallest positive-dt transition sd of the axis, coarsened uniformly where the product would exceed the point budget
(about 10^6 points: the budget, not the 1/6 rule, sets the spacing at d = 3).  A transition is a dense matrix per axis,
h_j N(x'_i; A x_j + b, q), from the old grid to the new one; the density is renormalised after every observation (and every
LGCP sub-step) with the normaliser accumulated into ll.  The mass the prediction puts outside the new grid is computed
exactly from the Gaussian tails and reported.

The error bound: the same computation with every spacing divided by 1.5; the bound is the absolute difference of the two
(likelihood, means, quantiles), and the finer result is the one returned.

The smoothers: the fixed-interval smoothing distributions p(x_s | y_1..T) that the rows of interpolate converge to (row 0 the initial
state at min(t), row s+1 the state at t[s]) -- `rts` in closed form for the Gaussian-observation models, `grid_smoother` /
`smoother_reference` by a backward pass over the grids and matrices the forward pass built, with the same error-bound conventions.

The predictive truth: what a forecast converges to (ParticleFilter.getForecast, :368-382: the cloud moved by stepFunction(t - s.t),
gamma = f(x, t), eta = link(gamma), an observation drawn from observation(gamma); horizon h continues horizon h - 1).
* `compose`: the transitions over several horizons compose in closed form into one (A, b, q) per component from the cloud's time;
  a repeated time adds the identity, so a later horizon's cumulative q stays positive.
* `predictive`: the filtering density on its grid convolved with that Gaussian.  Every statistic is then an integral of a SMOOTH
  function against the grid -- P(x_k <= c) = sum_j p_j Phi((c - A_k x_jk - b_k) / sqrt(q_k)), likewise gamma = H(t_h) . x (at
  d > 1 the grid's nodes are projected onto gamma and binned at 1/64 of the noise sd) -- which is why it is exact where a histogram
  of the grid would not be.  A horizon at the cloud's own time (q = 0) at the head of the list is refused by name: the integrand is
  not smooth there, and the filtering distribution itself is what GridResult holds.  Row 0 (the prior) is Gaussian and exact at any dt.
* `mixture_predictive`: M pairs (theta_m, x_m) at t0 are an M-component Gaussian mixture with per-pair (A_m, b_m, q_m): closed
  form at any latent dimension; with a variance per pair it is the prior.
* links and observation laws (`link_of`, `obs_mean_given`, `obs_cdf_given`) are written from Model.scala's leaves with
  scipy.stats, in the parametrisations of log_potential; E[eta], E[Y] and P(Y <= c) integrate them against gamma's mixture on
  a uniform axis.  Continuous kinds have a quantile function (the root of the mixture CDF), counts their CDF at the integers.
* the error bound is the module's: everything again at spacing / 1.5 (grid, binning and gamma axis), the absolute difference.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np
from scipy.special import expit, gammaln, ndtr

SDE_BROWNIAN, SDE_GEN_BROWNIAN, SDE_OU, SDE_EULER_AFFINE = 0, 1, 2, 3
POINT_BUDGET = 1_000_000
SD_COVER = 12.0
REFINE = 1.5
QUANTILES = (0.025, 0.975)


def _repeat(v, dim):
    v = np.asarray(v, dtype=np.float64)
    return v[np.arange(dim) % len(v)]


@dataclass
class Spec:
    """A model reduced to what the grid needs: per component the initial N(m0, c0), the transition kind and its constants, the
    observation model of the leftmost leaf, and how gamma reads the state."""
    m0: np.ndarray
    c0: np.ndarray
    kind: np.ndarray
    p1: np.ndarray          # sigma (Brownian, GenBrownian, OU) or g (Euler)
    p2: np.ndarray          # mu (GenBrownian, OU) or a (Euler)
    p3: np.ndarray          # phi (OU) or b (Euler)
    gamma_terms: List[Tuple[int, int, int]]    # (component, 0 = constant 1 / 1 = cos / 2 = sin, harmonic a * 2 pi / period as index)
    freqs: List[float]
    obs: str
    scale: float
    df: int

    @property
    def d(self):
        return len(self.m0)

    def transition(self, dt):
        """(A, b, q) per component for a step of length dt."""
        d = self.d
        A, b, q = np.ones(d), np.zeros(d), np.zeros(d)
        for k in range(d):
            kind, s, m, ph = self.kind[k], self.p1[k], self.p2[k], self.p3[k]
            if kind == SDE_BROWNIAN:
                q[k] = s * dt
            elif kind == SDE_GEN_BROWNIAN:
                b[k], q[k] = m * dt, s * dt
            elif kind == SDE_OU:
                A[k] = math.exp(-ph * dt)
                b[k] = m * (1.0 - A[k])
                q[k] = s * s * -math.expm1(-2.0 * ph * dt) / (2.0 * ph)
            else:
                A[k], b[k], q[k] = 1.0 + ph * dt, m * dt, s * s * dt
        return A, b, q

    def H(self, t):
        """gamma = H(t) . x."""
        h = np.zeros(self.d)
        for comp, fn, fi in self.gamma_terms:
            h[comp] = 1.0 if fn == 0 else (math.cos(self.freqs[fi] * t) if fn == 1 else math.sin(self.freqs[fi] * t))
        return h


def spec_of(model) -> Spec:
    """The host mirror's parameterised Model -> Spec, from its STORED parameters (SdeParameters.scala:192-205)."""
    m0, c0, kind, p1, p2, p3, terms, freqs = [], [], [], [], [], [], [], []
    base = 0
    for spec, node, sde in model.leaves:
        p, dim = sde.params, sde.dimension
        m0.append(_repeat(p.m0, dim))
        c0.append(np.exp(_repeat(p.c0, dim)))
        kind.append(np.full(dim, sde.kind))
        z = np.zeros(dim)
        if sde.kind == SDE_BROWNIAN:
            p1.append(np.exp(_repeat(p.sigma, dim))); p2.append(z); p3.append(z)
        elif sde.kind == SDE_GEN_BROWNIAN:
            p1.append(np.exp(_repeat(p.sigma, dim))); p2.append(_repeat(p.mu, dim)); p3.append(z)
        elif sde.kind == SDE_OU:
            p1.append(np.exp(_repeat(p.sigma, dim))); p2.append(_repeat(p.mu, dim)); p3.append(expit(_repeat(p.phi, dim)))
        else:
            p1.append(_repeat(p.g, dim)); p2.append(_repeat(p.a, dim)); p3.append(_repeat(p.b, dim))
        if spec.obs == "seasonal":
            for a in range(1, spec.harmonics + 1):
                freqs.append(2.0 * math.pi * a / spec.period)
                terms.append((base + 2 * a - 2, 1, len(freqs) - 1))
                terms.append((base + 2 * a - 1, 2, len(freqs) - 1))
        else:
            terms.append((base, 0, 0))
        base += dim
    first_spec, first_node = model.leaves[0][0], model.leaves[0][1]
    cat = lambda v: np.concatenate(v)
    return Spec(cat(m0), cat(c0), cat(kind).astype(int), cat(p1), cat(p2), cat(p3), terms, freqs, first_spec.obs,
                0.0 if first_node.scale is None else float(first_node.scale), int(first_spec.df))


# ------------------------------------------------------------------------------------------------ observation potentials
def log_potential(obs, scale, df, gamma, y):
    """log g(y | gamma) of the leftmost leaf, elementwise over gamma."""
    if obs == "poisson":                                         # breeze Poisson(exp(gamma)).logProbabilityOf(y.toInt)
        k = float(int(y))
        return k * gamma - np.exp(gamma) - gammaln(k + 1.0)
    if obs in ("linear", "seasonal"):                            # Gaussian(gamma, exp(scale)).logPdf(y)
        v = math.exp(scale)
        return -0.5 * math.log(2.0 * math.pi * v * v) - 0.5 * ((y - gamma) / v) ** 2
    if obs == "studentt":                                        # 1/v * StudentsT(df).logPdf((y - gamma) / v)
        v = math.exp(scale)
        z = (y - gamma) / v
        lp = gammaln((df + 1) / 2.0) - gammaln(df / 2.0) - 0.5 * math.log(df * math.pi) - (df + 1) / 2.0 * np.log1p(z * z / df)
        return lp / v
    if obs == "negbin":                                          # size = exp(scale), mu = exp(gamma)
        size, k = math.exp(scale), float(int(y))
        lse = np.logaddexp(gamma, scale)                         # log(mu + size)
        return gammaln(size + k) - gammaln(k + 1.0) - gammaln(size) + size * (scale - lse) + k * (gamma - lse)
    if obs == "zip":                                             # p = logistic(scale) of structural zeros
        p, k = expit(scale), int(y)
        if k == 0:
            return np.log(p + (1.0 - p) * np.exp(-np.exp(gamma)))
        return -np.logaddexp(0.0, scale) + k * gamma - np.exp(gamma) - gammaln(k + 1.0)
    if obs == "bernoulli":                                       # link clamped at +-6, -1e99 where the log would be of 0
        link = np.where(gamma > 6, 1.0, np.where(gamma < -6, 0.0, expit(gamma)))
        with np.errstate(divide="ignore"):
            if y == 1.0:
                return np.where(link == 0.0, -1e99, np.log(link))
            return np.where(link == 1.0, -1e99, np.log(1.0 - link))
    if obs == "beta":                                            # Beta(exp(-gamma), 1).logPdf(y) = log a + (a - 1) log y
        a = np.exp(-gamma)
        return -gamma + (a - 1.0) * math.log(y)
    raise ValueError(obs)


# ------------------------------------------------------------------------------------------------ the grid
class _Grid:
    def __init__(self, axes: List[np.ndarray], p: np.ndarray):
        self.axes, self.p = axes, p                               # p: density values; integrals are sum(p) * vol

    @property
    def h(self):
        return np.array([a[1] - a[0] for a in self.axes])

    @property
    def vol(self):
        return float(np.prod(self.h))

    def marginal(self, k):
        other = tuple(i for i in range(len(self.axes)) if i != k)
        h = self.h
        return self.p.sum(axis=other) * float(np.prod([h[i] for i in other])) if other else self.p.copy()

    def moments(self):
        m, v = [], []
        for k, a in enumerate(self.axes):
            f = self.marginal(k) * self.h[k]
            tot = f.sum()
            mu = float((f * a).sum() / tot)
            m.append(mu)
            v.append(float((f * (a - mu) ** 2).sum() / tot))
        return np.array(m), np.array(v)

    def gamma(self, H):
        g = 0.0
        for k, a in enumerate(self.axes):
            shape = [1] * len(self.axes); shape[k] = len(a)
            if H[k] != 0.0:
                g = g + H[k] * a.reshape(shape)
        return g

    def apply_axis(self, k, K):
        return np.moveaxis(np.tensordot(K, self.p, axes=([1], [k])), 0, k)


def _axis(mean, sd, h):
    n = int(math.ceil(2.0 * SD_COVER * sd / h)) + 1
    return mean - 0.5 * (n - 1) * h + h * np.arange(n)


def _spacing(sds, h_rule, budget):
    """Per-axis spacing: the rule, coarsened uniformly until the grid covering +-SD_COVER sds fits the budget."""
    h = np.array(h_rule, dtype=np.float64)
    n = np.ceil(2.0 * SD_COVER * np.asarray(sds) / h) + 1
    tot = float(np.prod(n))
    if tot > budget:
        h = h * (tot / budget) ** (1.0 / len(h)) * 1.0001
    return h


@dataclass
class GridResult:
    ll_t: np.ndarray                 # cumulative log-likelihood after each datum
    mean: np.ndarray                 # [T, d] filtering means
    lo: np.ndarray                   # [T, d] 2.5 % quantiles
    hi: np.ndarray                   # [T, d] 97.5 % quantiles
    lost: float                      # largest prediction mass that fell outside a new grid
    points: int                      # largest grid used
    h_over_sd: float                 # largest spacing / smallest transition sd used
    ll_err: np.ndarray = field(default=None)      # refinement bounds (filled by `reference`)
    mean_err: np.ndarray = field(default=None)
    lo_err: np.ndarray = field(default=None)
    hi_err: np.ndarray = field(default=None)

    @property
    def ll(self):
        return float(self.ll_t[-1])


def _quantiles(a, f, qs, up=64):
    """Quantiles of the smooth density f sampled on the uniform axis a: band-limited (FFT) upsampling of f by `up`, then the
    trapezoid CDF and linear interpolation on the fine axis."""
    n = len(a)
    pad = 2 * n
    F = np.fft.rfft(np.concatenate([f, np.zeros(pad - n)]))
    fine = np.fft.irfft(F, pad * up)[: (n - 1) * up + 1] * up
    fine = np.maximum(fine, 0.0)
    x = a[0] + (a[1] - a[0]) / up * np.arange(len(fine))
    c = np.concatenate([[0.0], np.cumsum(0.5 * (fine[1:] + fine[:-1]))])
    c /= c[-1]
    return [float(np.interp(q, c, x)) for q in qs]


def grid_filter(spec: Spec, t, y, has, lgcp_precision=0, refine=1.0, budget=POINT_BUDGET, keep=None) -> GridResult:
    """`keep`: a list that receives what a backward pass needs (grid_smoother) -- first (axes, density) of the initial state, then
    per datum (axes, post-observation density, per-axis matrices of the move or None, potential or None).  The filter's own
    arithmetic does not depend on it."""
    t = np.asarray(t, dtype=np.float64); y = np.asarray(y, dtype=np.float64)
    has = np.ones(len(t), dtype=bool) if has is None else np.asarray(has).astype(bool)
    d, lgcp = spec.d, spec.obs == "lgcp"
    if d > 3:
        raise ValueError("the grid filter covers latent dimensions up to 3")
    delta = 10.0 ** -lgcp_precision if lgcp else None
    # the spacing rule: 1/6 of the smallest one-step transition sd per axis (sub-steps of delta for the LGCP)
    dts = [delta] if lgcp else [x for x in np.diff(np.concatenate([[t.min()], t])) if x > 0]
    qmin = np.min([spec.transition(x)[2] for x in dts], axis=0) if dts else spec.c0
    h_rule = np.sqrt(np.minimum(qmin, spec.c0)) / 6.0 / refine
    sd0 = np.sqrt(spec.c0)
    h = _spacing(sd0, h_rule, budget)
    axes = [_axis(spec.m0[k], sd0[k], h[k]) for k in range(d)]
    dens = 1.0
    for k in range(d):
        shape = [1] * d; shape[k] = len(axes[k])
        dens = dens * (np.exp(-0.5 * (axes[k] - spec.m0[k]) ** 2 / spec.c0[k]) / math.sqrt(2 * math.pi * spec.c0[k])).reshape(shape)
    G = _Grid(axes, np.array(dens))
    G.p /= G.p.sum() * G.vol
    lost, points, hos = 2 * d * float(ndtr(-SD_COVER)), G.p.size, 0.0

    def move(G, dt):
        nonlocal lost, points, hos
        A, b, q = spec.transition(dt)
        m, v = G.moments()
        pm, pv = A * m + b, A * A * v + q
        hn = _spacing(np.sqrt(pv), h_rule, budget)
        hos = max(hos, float(np.max(hn / np.sqrt(q))))
        new_axes, p, out, Ks = [], G.p, 0.0, []
        for k in range(d):
            ax = _axis(pm[k], math.sqrt(pv[k]), hn[k])
            src = G.axes[k]
            mu = A[k] * src + b[k]
            s = math.sqrt(q[k])
            K = np.exp(-0.5 * ((ax[:, None] - mu[None, :]) / s) ** 2) / (s * math.sqrt(2 * math.pi)) * (src[1] - src[0])
            p = np.moveaxis(np.tensordot(K, p, axes=([1], [k])), 0, k)
            # the exact Gaussian mass each source point sends outside [ax0 - h/2, axN + h/2], weighted by the source marginal
            tail = ndtr((ax[0] - 0.5 * hn[k] - mu) / s) + ndtr((mu - ax[-1] - 0.5 * hn[k]) / s)
            out += float((G.marginal(k) * (src[1] - src[0]) * tail).sum())
            new_axes.append(ax)
            Ks.append(K)
        lost = max(lost, out)
        Gn = _Grid(new_axes, p)
        points = max(points, p.size)
        return Gn, Ks

    def normalise(G):
        z = float(G.p.sum()) * G.vol
        G.p /= z
        return math.log(z)

    T = len(t)
    ll, now = 0.0, float(t.min())
    ll_t, mean, lo, hi = np.zeros(T), np.zeros((T, d)), np.zeros((T, d)), np.zeros((T, d))
    if keep is not None:
        if lgcp:
            raise ValueError("no backward pass for the LGCP: interpolate refuses it")
        keep.append((G.axes, G.p))
    for s in range(T):
        Ks, pot = None, None
        dt = float(t[s]) - now
        if lgcp:
            if dt != 0:
                nsub = int(math.ceil(dt / delta))
                tau = float(t[s])
                for _ in range(nsub):
                    G = move(G, delta)[0]
                    tau = tau + delta
                    G.p *= np.exp(-np.exp(G.gamma(spec.H(tau))) * delta)
                    ll += normalise(G)
                G.p *= np.exp(G.gamma(spec.H(float(t[s]))))
                ll += normalise(G)
        else:
            if dt != 0:
                G, Ks = move(G, dt)
            if has[s]:
                lg = log_potential(spec.obs, spec.scale, spec.df, G.gamma(spec.H(float(t[s]))), float(y[s]))
                mx = float(np.max(lg))
                pot = np.exp(lg - mx)
                G.p = G.p * pot
                ll += mx + normalise(G)
        now = float(t[s])
        ll_t[s] = ll
        mean[s] = G.moments()[0]
        for k in range(d):
            lo[s, k], hi[s, k] = _quantiles(G.axes[k], G.marginal(k), QUANTILES)
        if keep is not None:                                       # (no kept array is written in place afterwards)
            keep.append((G.axes, G.p, Ks, pot))
    return GridResult(ll_t, mean, lo, hi, lost, points, hos)


_CACHE: Dict[tuple, GridResult] = {}


def _key(model, t, y, has, lgcp_precision):
    leaves = tuple((spec.obs, spec.period, spec.harmonics, spec.df, node.scale, sde.kind, sde.dimension,
                    tuple(node.sdeParam.flatten())) for spec, node, sde in model.leaves)
    has_b = b"" if has is None else np.asarray(has, dtype=np.uint8).tobytes()
    return (leaves, np.asarray(t, np.float64).tobytes(), np.asarray(y, np.float64).tobytes(), has_b, int(lgcp_precision))


def reference(model, t, y, has=None, lgcp_precision=0, budget=POINT_BUDGET) -> GridResult:
    """The grid filter at spacing h and h / 1.5; returns the finer result with the absolute differences as its error bounds.
    Cached per (model, series)."""
    key = _key(model, t, y, has, lgcp_precision) + (budget,)
    if key not in _CACHE:
        spec = spec_of(model)
        a = grid_filter(spec, t, y, has, lgcp_precision, 1.0, budget)
        b = grid_filter(spec, t, y, has, lgcp_precision, REFINE, budget=budget * REFINE ** spec.d)
        b.ll_err = np.abs(b.ll_t - a.ll_t)
        b.mean_err = np.abs(b.mean - a.mean)
        # (the quantiles add a linear interpolation of the CDF whose error is not monotone in h: three times the difference,
        #  and a floor of 1e-5 -- measured against Kalman at d = 1 and 3: 1e-6 and 8e-6)
        b.lo_err, b.hi_err = 3.0 * np.abs(b.lo - a.lo) + 1e-5, 3.0 * np.abs(b.hi - a.hi) + 1e-5
        b.lost = max(a.lost, b.lost)
        _CACHE[key] = b
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ closed form
def kalman(spec: Spec, t, y, has=None):
    """The d-dimensional Kalman filter of a Gaussian-observation model (H(t) from the leaves, every transition kind):
    (ll_t, filtering means [T, d], filtering variances [T, d])."""
    if spec.obs not in ("linear", "seasonal"):
        raise ValueError("Kalman needs a Gaussian observation")
    t = np.asarray(t, dtype=np.float64)
    has = np.ones(len(t), dtype=bool) if has is None else np.asarray(has).astype(bool)
    r = math.exp(spec.scale) ** 2
    m, P = spec.m0.copy(), np.diag(spec.c0)
    now, ll = float(t.min()), 0.0
    T = len(t)
    ll_t, means, vars_ = np.zeros(T), np.zeros((T, spec.d)), np.zeros((T, spec.d))
    for s in range(T):
        dt = float(t[s]) - now
        if dt != 0:
            A, b, q = spec.transition(dt)
            m = A * m + b
            P = A[:, None] * P * A[None, :] + np.diag(q)
        if has[s]:
            H = spec.H(float(t[s]))
            S = float(H @ P @ H) + r
            e = float(y[s]) - float(H @ m)
            ll += -0.5 * (math.log(2 * math.pi * S) + e * e / S)
            K = P @ H / S
            m = m + K * e
            P = P - np.outer(K, H @ P)
        now = float(t[s])
        ll_t[s], means[s], vars_[s] = ll, m, np.diag(P)
    return ll_t, means, vars_


def _gaussian_forward(spec: Spec, t, y, has):
    """The forward pass of `kalman` with what a backward pass needs kept: filtering means [T+1, d] and full covariances
    [T+1, d, d] (row 0 the initial state at min(t), row s+1 after datum s) and each step's (A, b, q)."""
    if spec.obs not in ("linear", "seasonal"):
        raise ValueError("Kalman needs a Gaussian observation")
    t = np.asarray(t, dtype=np.float64)
    has = np.ones(len(t), dtype=bool) if has is None else np.asarray(has).astype(bool)
    r = math.exp(spec.scale) ** 2
    d, T = spec.d, len(t)
    m, P = spec.m0.copy(), np.diag(spec.c0)
    now = float(t.min())
    means, covs, steps = np.zeros((T + 1, d)), np.zeros((T + 1, d, d)), []
    means[0], covs[0] = m, P
    for s in range(T):
        dt = float(t[s]) - now
        A, b, q = spec.transition(dt) if dt != 0 else (np.ones(d), np.zeros(d), np.zeros(d))   # dt = 0 is the identity
        m = A * m + b
        P = A[:, None] * P * A[None, :] + np.diag(q)
        if has[s]:
            H = spec.H(float(t[s]))
            S = float(H @ P @ H) + r
            K = P @ H / S
            m = m + K * (float(y[s]) - float(H @ m))
            P = P - np.outer(K, H @ P)
            P = 0.5 * (P + P.T)
        now = float(t[s])
        means[s + 1], covs[s + 1] = m, P
        steps.append((A, b, q))
    return means, covs, steps


def rts(spec: Spec, t, y, has=None):
    """The Rauch-Tung-Striebel fixed-interval smoother of a Gaussian-observation model: smoothed means [T+1, d] and full
    covariances [T+1, d, d] of p(x_s | y_1..T); row 0 is the initial state at min(t), row s+1 the state at t[s]."""
    mf, Pf, steps = _gaussian_forward(spec, t, y, has)
    ms, Ps = mf.copy(), Pf.copy()
    for s in range(len(steps) - 1, -1, -1):
        A, b, q = steps[s]
        mp = A * mf[s] + b
        Pp = A[:, None] * Pf[s] * A[None, :] + np.diag(q)
        G = np.linalg.solve(Pp, A[:, None] * Pf[s]).T              # P_f A' Pp^-1 (both symmetric)
        ms[s] = mf[s] + G @ (ms[s + 1] - mp)
        Ps[s] = Pf[s] + G @ (Ps[s + 1] - Pp) @ G.T
        Ps[s] = 0.5 * (Ps[s] + Ps[s].T)
    return ms, Ps


def gamma_moments(spec: Spec, mean, cov, time):
    """Mean and sd of gamma = H(time) . x for x ~ N(mean, cov)."""
    H = spec.H(float(time))
    return float(H @ mean), math.sqrt(float(H @ cov @ H))


# ------------------------------------------------------------------------------------------------ the grid smoother
@dataclass
class SmoothResult:
    mean: np.ndarray                 # [T+1, d] smoothed means; row 0 the initial state at min(t), row s+1 the state at t[s]
    lo: np.ndarray                   # [T+1, d] 2.5 % marginal quantiles
    hi: np.ndarray                   # [T+1, d] 97.5 % marginal quantiles
    filter: GridResult               # the forward pass: exactly what grid_filter returns
    mean_err: np.ndarray = field(default=None)    # refinement bounds (filled by `smoother_reference`)
    lo_err: np.ndarray = field(default=None)
    hi_err: np.ndarray = field(default=None)


def grid_smoother(spec: Spec, t, y, has, refine=1.0, budget=POINT_BUDGET) -> SmoothResult:
    """The fixed-interval smoothing distributions p(x_s | y_1..T) on the grids of grid_filter: its forward pass, then
    beta_T = 1, beta_s(x) = sum_i N(x'_i; A x + b, q) h'_i g_s(x'_i) beta_{s+1}(x'_i) per axis (the forward matrices
    transposed, with the new grid's spacing in place of the old one's), renormalised by its maximum;
    smoothed_s = filtered_s beta_s."""
    if spec.obs == "lgcp":
        raise ValueError("no smoother for the LGCP: interpolate refuses it")
    keep = []
    f = grid_filter(spec, t, y, has, 0, refine, budget, keep=keep)
    T, d = len(keep) - 1, spec.d
    mean, lo, hi = np.zeros((T + 1, d)), np.zeros((T + 1, d)), np.zeros((T + 1, d))

    def summarise(row, axes, p):
        G = _Grid(axes, p)
        mean[row] = G.moments()[0]
        for k in range(d):
            lo[row, k], hi[row, k] = _quantiles(axes[k], G.marginal(k), QUANTILES)

    beta = np.ones_like(keep[T][1])
    summarise(T, keep[T][0], keep[T][1])
    for s in range(T - 1, -1, -1):                                  # the step from row s to row s + 1 is datum s
        axes_new, _, Ks, pot = keep[s + 1]
        axes_old, p_old = keep[s][0], keep[s][1]
        keep[s + 1] = None
        if pot is not None:
            beta = beta * pot
        if Ks is not None:
            for k in range(d):
                B = Ks[k].T * ((axes_new[k][1] - axes_new[k][0]) / (axes_old[k][1] - axes_old[k][0]))
                beta = np.moveaxis(np.tensordot(B, beta, axes=([1], [k])), 0, k)
        beta = beta / float(np.max(beta))
        summarise(s, axes_old, p_old * beta)
    return SmoothResult(mean, lo, hi, f)


_SMOOTH_CACHE: Dict[tuple, SmoothResult] = {}


def smoother_reference(model, t, y, has=None, budget=POINT_BUDGET) -> SmoothResult:
    """The grid smoother at spacing h and h / 1.5; returns the finer result with error bounds by `reference`'s conventions
    (means: the absolute difference; quantiles: three times the difference + 1e-5), its `filter` with `reference`'s bounds.
    Cached per (model, series)."""
    key = _key(model, t, y, has, 0) + (budget,)
    if key not in _SMOOTH_CACHE:
        spec = spec_of(model)
        a = grid_smoother(spec, t, y, has, 1.0, budget)
        b = grid_smoother(spec, t, y, has, REFINE, budget=budget * REFINE ** spec.d)
        b.mean_err = np.abs(b.mean - a.mean)
        b.lo_err, b.hi_err = 3.0 * np.abs(b.lo - a.lo) + 1e-5, 3.0 * np.abs(b.hi - a.hi) + 1e-5
        fa, fb = a.filter, b.filter
        fb.ll_err = np.abs(fb.ll_t - fa.ll_t)
        fb.mean_err = np.abs(fb.mean - fa.mean)
        fb.lo_err, fb.hi_err = 3.0 * np.abs(fb.lo - fa.lo) + 1e-5, 3.0 * np.abs(fb.hi - fa.hi) + 1e-5
        fb.lost = max(fa.lost, fb.lost)
        _SMOOTH_CACHE[key] = b
    return _SMOOTH_CACHE[key]


# ------------------------------------------------------------------------------------------------ the predictive truth
# Written from Model.scala's link / observation of each leaf (:145-345) and ParticleFilter.getForecast (:368-382): the state is
# moved by stepFunction(t - s.t), gamma = f(x, t), eta = link(gamma), the observation is drawn from observation(gamma) -- with
# scipy.stats for every law, in the parametrisations of log_potential above and tests/golden/make_golden.py.
COUNT_KINDS = ("poisson", "negbin", "zip", "bernoulli")


def link_of(obs, gamma):
    """eta = link(gamma) of the leftmost leaf, elementwise."""
    gamma = np.asarray(gamma, dtype=np.float64)
    if obs in ("poisson", "negbin", "zip"):
        return np.exp(gamma)
    if obs in ("linear", "seasonal", "studentt"):
        return gamma
    if obs == "bernoulli":
        return np.where(gamma > 6, 1.0, np.where(gamma < -6, 0.0, expit(gamma)))
    if obs == "beta":
        return np.exp(-gamma)
    raise ValueError(obs)


def link_decreases(obs):
    return obs == "beta"


def obs_mean_given(obs, scale, df, eta):
    """E[Y | eta], elementwise."""
    if obs in ("poisson", "negbin", "bernoulli", "linear", "seasonal"):
        return eta
    if obs == "studentt":
        if df <= 1:
            raise ValueError("a Student-t with df <= 1 has no mean")
        return eta
    if obs == "zip":
        return (1.0 - expit(scale)) * eta
    if obs == "beta":                                            # Beta(eta, scale): the stored scale as it is
        return eta / (eta + scale)
    raise ValueError(obs)


def obs_cdf_given(obs, scale, df, eta, c):
    """P(Y <= c | eta) by scipy.stats, broadcasting eta against c."""
    from scipy import stats
    if obs == "poisson":
        return stats.poisson.cdf(c, eta)
    if obs in ("linear", "seasonal"):
        return stats.norm.cdf(c, eta, math.exp(scale))
    if obs == "studentt":
        return stats.t.cdf(c, df, loc=eta, scale=math.exp(scale))
    if obs == "negbin":
        size = math.exp(scale)
        return stats.nbinom.cdf(c, size, size / (size + eta))
    if obs == "zip":
        p = expit(scale)
        return p * (np.asarray(c) >= 0) + (1.0 - p) * stats.poisson.cdf(c, eta)
    if obs == "bernoulli":
        return stats.bernoulli.cdf(c, eta)
    if obs == "beta":
        return stats.beta.cdf(c, eta, scale)
    raise ValueError(obs)


def compose(spec: Spec, t0, times):
    """The cumulative (A, b, q) per component from t0 to each horizon, horizon h continuing horizon h - 1 (which matters for the
    Euler-Maruyama step, whose two steps are not one step of the sum); a repeated time adds the identity."""
    d = spec.d
    A, b, q = np.ones(d), np.zeros(d), np.zeros(d)
    now, out = float(t0), []
    for th in times:
        dt = float(th) - now
        if dt < 0:
            raise ValueError("horizon times must not decrease, nor precede the cloud's time")
        if dt != 0:
            A1, b1, q1 = spec.transition(dt)
            A, b, q = A1 * A, A1 * b + b1, A1 * A1 * q + q1
        now = float(th)
        out.append((A.copy(), b.copy(), q.copy()))
    return out


class GaussMix:
    """A one-dimensional Gaussian mixture sum_j w_j N(mu_j, var_j), every var_j > 0."""

    def __init__(self, mu, w, var):
        self.mu = np.atleast_1d(np.asarray(mu, dtype=np.float64))
        self.w = np.broadcast_to(np.asarray(w, dtype=np.float64), self.mu.shape).copy()
        self.sd = np.sqrt(np.broadcast_to(np.asarray(var, dtype=np.float64), self.mu.shape))
        if not np.all(self.sd > 0):
            raise ValueError("dt = 0 predictive: a component without transition noise is not a smooth integrand")

    def mean(self):
        return float((self.w * self.mu).sum() / self.w.sum())

    def cdf(self, c):
        c = np.asarray(c, dtype=np.float64)
        return (self.w * ndtr((c[..., None] - self.mu) / self.sd)).sum(axis=-1) / self.w.sum()

    def pdf(self, c):
        z = (np.asarray(c, dtype=np.float64)[..., None] - self.mu) / self.sd
        return (self.w / self.sd * np.exp(-0.5 * z * z)).sum(axis=-1) / (math.sqrt(2 * math.pi) * self.w.sum())

    def span(self, k=SD_COVER):
        return float(np.min(self.mu - k * self.sd)), float(np.max(self.mu + k * self.sd))

    def quantile(self, p):
        from scipy.optimize import brentq
        lo, hi = self.span()
        return float(brentq(lambda c: float(self.cdf(c)) - p, lo, hi, xtol=1e-13, rtol=1e-14))

    @staticmethod
    def join(parts, weights):
        return GaussMix(np.concatenate([m.mu for m in parts]), np.concatenate([wt * m.w / m.w.sum() for m, wt in zip(parts, weights)]),
                        np.concatenate([m.sd ** 2 for m in parts]))


@dataclass
class _Group:
    """A share of the predictive under one parameter set: its weight, its observation law and its mixture of gamma."""
    weight: float
    obs: str
    scale: float
    df: int
    gamma: GaussMix


class Horizon:
    """The exact predictive at one horizon: a Gaussian mixture per state component, and per parameter set a mixture of gamma that
    the link and the observation law are integrated against on a uniform axis (spacing 1/8 of the smallest component sd, divided
    by `refine`: the integrand is smooth, so the sum converges faster than any power of the spacing)."""

    def __init__(self, state: List[GaussMix], groups: List[_Group], refine=1.0):
        self.state, self.groups, self.refine = state, groups, refine
        tot = sum(g.weight for g in groups)
        for g in groups:
            g.weight = g.weight / tot
        self.obs = groups[0].obs
        self.gamma = groups[0].gamma if len(groups) == 1 else GaussMix.join([g.gamma for g in groups], [g.weight for g in groups])
        self._quad = None

    def quad(self):
        """per group (gamma axis, probability of each node)"""
        if self._quad is None:
            self._quad = []
            for g in self.groups:
                lo, hi = g.gamma.span(10.0)
                h = float(np.min(g.gamma.sd)) / 8.0 / self.refine
                n = int(math.ceil((hi - lo) / h)) + 1
                if n > 400_000:
                    raise ValueError("the gamma axis of this predictive would need %d nodes" % n)
                gg = lo + h * np.arange(n)
                pg = np.zeros(n)
                for i in range(0, n, 4096):                       # (blocks: the pdf is a [nodes, components] array)
                    pg[i:i + 4096] = g.gamma.pdf(gg[i:i + 4096]) * h
                self._quad.append((gg, pg))
        return self._quad

    def state_mean(self):
        return np.array([m.mean() for m in self.state])

    def state_quantile(self, p):
        p = np.broadcast_to(np.asarray(p, dtype=np.float64), (len(self.state),))
        return np.array([m.quantile(float(pk)) for m, pk in zip(self.state, p)])

    def gamma_mean(self):
        return self.gamma.mean()

    def eta_mean(self):
        return float(sum(g.weight * float((pg * link_of(g.obs, gg)).sum()) for g, (gg, pg) in zip(self.groups, self.quad())))

    def eta_quantile(self, p):
        return float(link_of(self.obs, self.gamma.quantile(1.0 - p if link_decreases(self.obs) else p)))

    def obs_mean(self):
        return float(sum(g.weight * float((pg * obs_mean_given(g.obs, g.scale, g.df, link_of(g.obs, gg))).sum())
                         for g, (gg, pg) in zip(self.groups, self.quad())))

    def obs_cdf(self, c):
        c = np.atleast_1d(np.asarray(c, dtype=np.float64))
        out = np.zeros(c.shape)
        for g, (gg, pg) in zip(self.groups, self.quad()):
            keep = pg > 0
            F = obs_cdf_given(g.obs, g.scale, g.df, link_of(g.obs, gg[keep])[None, :], c[:, None])
            out += g.weight * (F * pg[keep][None, :]).sum(axis=1)
        return out

    def obs_quantile(self, p):
        """continuous kinds: the root of the mixture CDF"""
        from scipy.optimize import brentq
        if self.obs in COUNT_KINDS:
            raise ValueError("a count has an integer quantile: obs_int_quantile")
        if self.obs == "beta":
            lo, hi = 0.0, 1.0
        else:
            lo, hi = self.gamma.span()
            w = 10.0 * math.exp(self.groups[0].scale)
            while float(self.obs_cdf(lo)[0]) > p:
                lo -= w; w *= 2
            w = 10.0 * math.exp(self.groups[0].scale)
            while float(self.obs_cdf(hi)[0]) < p:
                hi += w; w *= 2
        return float(brentq(lambda c: float(self.obs_cdf(c)[0]) - p, lo, hi, xtol=1e-12, rtol=1e-13))

    def obs_int_cdf(self, kmax=None):
        """counts: (integers 0..K, their CDF), K the first integer whose CDF passes 1 - 1e-5 (or kmax): every probability a test
        looks up lies below 0.9995 + its margin"""
        K = 64 if kmax is None else max(int(kmax), 1)
        while True:
            k = np.arange(K + 1)
            F = self.obs_cdf(k)
            if kmax is not None or F[-1] >= 1.0 - 1e-5 or self.obs == "bernoulli":
                break
            K *= 2
        if self.obs == "bernoulli":
            return k[:2], F[:2]
        if kmax is not None:
            return k[:kmax + 1], F[:kmax + 1]
        last = int(np.argmax(F >= 1.0 - 1e-5))
        return k[:last + 1], F[:last + 1]

    def obs_int_quantile(self, p, table=None):
        """the exact integer quantile function: the smallest k with P(Y <= k) >= p"""
        k, F = table if table is not None else self.obs_int_cdf()
        i = int(np.searchsorted(F, p, side="left"))
        return int(k[min(i, len(k) - 1)])


class Predictive:
    """The predictive at spacing h (`coarse`) and h / 1.5 (`fine`): every statistic is returned from the finer one together with
    the absolute difference of the two as its error bound."""

    def __init__(self, times, coarse: List[Horizon], fine: List[Horizon]):
        self.times, self.coarse, self.fine = np.asarray(times, dtype=np.float64), coarse, fine
        self.d = len(fine[0].state)
        self.obs = fine[0].obs

    def _both(self, f):
        a = np.array([f(h) for h in self.coarse], dtype=np.float64)
        b = np.array([f(h) for h in self.fine], dtype=np.float64)
        return b, np.abs(b - a)

    def state_mean(self):                                        # ([H, d], err)
        return self._both(lambda h: h.state_mean())

    def state_quantile(self, p):
        return self._both(lambda h: h.state_quantile(p))

    def gamma_mean(self):
        return self._both(lambda h: h.gamma_mean())

    def eta_mean(self):                                          # ([H], err)
        return self._both(lambda h: h.eta_mean())

    def eta_quantile(self, p):
        return self._both(lambda h: h.eta_quantile(p))

    def gamma_quantile(self, p):
        return self._both(lambda h: h.gamma.quantile(p))

    def obs_mean(self):
        return self._both(lambda h: h.obs_mean())

    def obs_quantile(self, p):
        return self._both(lambda h: h.obs_quantile(p))

    def obs_cdf(self, h, c):                                     # ([len(c)], err) at horizon h
        a, b = self.coarse[h].obs_cdf(c), self.fine[h].obs_cdf(c)
        return b, np.abs(b - a)

    def obs_int_cdf(self, h):                                    # (integers, CDF, err)
        k, F = self.fine[h].obs_int_cdf()
        _, Fa = self.coarse[h].obs_int_cdf(kmax=int(k[-1]))
        return k, F, np.abs(F - Fa)


@dataclass
class _Row:
    """A filtering density reduced to what a predictive reads: the axes, the marginal probabilities per axis and the nodes that
    carry mass (all but 1e-13 of it) as flat indices with their probabilities."""
    axes: List[np.ndarray]
    marg: List[np.ndarray]
    shape: tuple
    idx: np.ndarray
    p: np.ndarray


_ROWS: Dict[tuple, tuple] = {}


def _rows_of(spec, t, y, has, refine, budget):
    keep = []
    grid_filter(spec, t, y, has, 0, refine, budget, keep=keep)
    rows = []
    for entry in keep:
        G = _Grid(entry[0], entry[1])
        marg = []
        for k in range(spec.d):
            f = G.marginal(k) * G.h[k]
            marg.append(f / f.sum())
        flat = G.p.ravel()
        idx = np.flatnonzero(flat > flat.max() * 1e-14 / max(1.0, flat.size / 1e3))
        p = flat[idx]
        rows.append(_Row(G.axes, marg, G.p.shape, idx.astype(np.int64), p / p.sum()))
    return rows


def filtering_rows(model, t, y, has=None, budget=POINT_BUDGET):
    """The filtering densities of `reference` (row 0 the initial state, row s + 1 after datum s) at both spacings; cached."""
    key = _key(model, t, y, has, 0) + (budget,)
    if key not in _ROWS:
        spec = spec_of(model)
        _ROWS[key] = (_rows_of(spec, t, y, has, 1.0, budget), _rows_of(spec, t, y, has, REFINE, budget * REFINE ** spec.d))
    return _ROWS[key]


def _bin(u, w, width):
    """Weighted points moved onto a uniform axis of the given width, each shared between its two neighbours in proportion
    (mass and mean are kept; the variance added is at most width^2 / 4)."""
    lo = float(u.min())
    pos = (u - lo) / width
    i = np.floor(pos).astype(np.int64)
    f = pos - i
    n = int(i.max()) + 2
    acc = np.bincount(i, weights=w * (1.0 - f), minlength=n) + np.bincount(i + 1, weights=w * f, minlength=n)
    nz = np.flatnonzero(acc > 0)
    return lo + width * nz, acc[nz]


def _horizons_from_row(spec: Spec, row: _Row, t_row, times, refine):
    out = []
    d = spec.d
    for (A, b, q), th in zip(compose(spec, t_row, times), times):
        if not np.all(q > 0):
            raise ValueError("dt = 0 predictive from a grid: the integrand is not smooth; ask for a later time or the filtering "
                             "distribution itself (GridResult)")
        state = [GaussMix(A[k] * row.axes[k] + b[k], row.marg[k], q[k]) for k in range(d)]
        H = spec.H(float(th))
        Q = float((H * H * q).sum())
        if d == 1:
            gm = GaussMix(H[0] * (A[0] * row.axes[0] + b[0]), row.marg[0], Q)
        else:
            sub = np.unravel_index(row.idx, row.shape)
            u = np.zeros(len(row.idx))
            for k in range(d):
                if H[k] != 0.0:
                    u += H[k] * (A[k] * row.axes[k][sub[k]] + b[k])
            # (the nodes of the joint grid projected onto gamma: binned at 1/64 of the noise sd, finer with `refine`, so the
            #  refinement difference bounds the binning as well: its error in a CDF is at most 0.24 width^2 / (8 Q) = 7e-6)
            mu, w = _bin(u, row.p, math.sqrt(Q) / 64.0 / refine)
            gm = GaussMix(mu, w, Q)
        out.append(Horizon(state, [_Group(1.0, spec.obs, spec.scale, spec.df, gm)], refine))
    return out


def predictive(model, t, y, has, times, row=None, budget=POINT_BUDGET) -> Predictive:
    """The exact predictive distributions at `times` given the records up to row `row` of the filtering rows (default: all of
    them; row s + 1 is the state after datum s, row 0 the prior at min(t)): the filtering density on its grid convolved with the
    closed-form transition to each horizon.  Row 0 is the Gaussian prior itself (`mixture_predictive`), at any dt >= 0."""
    spec = spec_of(model)
    t = np.asarray(t, dtype=np.float64)
    if spec.obs == "lgcp":
        raise ValueError("no forecast for the LGCP")
    row = len(t) if row is None else row
    if row == 0:
        return mixture_predictive([(model, spec.m0, spec.c0)], float(t.min()), times)
    a, b = filtering_rows(model, t, y, has, budget)
    t_row = float(t[row - 1])
    return Predictive(times, _horizons_from_row(spec, a[row], t_row, times, 1.0), _horizons_from_row(spec, b[row], t_row, times, REFINE))


def mixture_predictive(pairs, t0, times, weights=None) -> Predictive:
    """The closed-form predictive of M pairs (model_m, x_m[, var_m]) at t0: per pair the state at a horizon is
    N(A_m x_m + b_m, A_m^2 var_m + q_m) per component (var_m = 0: a point; the prior: x = m0, var = c0), gamma Gaussian likewise,
    and the predictive is their mixture (equal weights unless given).  Exact at any latent dimension; only the link and the
    observation law are integrated numerically (Horizon), which is what the two refinements differ in."""
    M = len(pairs)
    weights = np.full(M, 1.0 / M) if weights is None else np.asarray(weights, dtype=np.float64) / np.sum(weights)
    specs = [spec_of(p[0]) for p in pairs]
    comps = [compose(s, t0, times) for s in specs]
    d = specs[0].d

    def build(refine):
        out = []
        for h, th in enumerate(times):
            mus, vs, groups = np.zeros((M, d)), np.zeros((M, d)), []
            for m, (pair, spec) in enumerate(zip(pairs, specs)):
                x = np.asarray(pair[1], dtype=np.float64)
                v0 = np.zeros(d) if len(pair) < 3 else np.asarray(pair[2], dtype=np.float64)
                A, b, q = comps[m][h]
                mus[m], vs[m] = A * x + b, A * A * v0 + q
                H = spec.H(float(th))
                groups.append(_Group(float(weights[m]), spec.obs, spec.scale, spec.df,
                                     GaussMix([float(H @ mus[m])], [1.0], [float((H * H * vs[m]).sum())])))
            state = [GaussMix(mus[:, k], weights, vs[:, k]) for k in range(d)]
            out.append(Horizon(state, groups, refine))
        return out
    return Predictive(times, build(1.0), build(REFINE))
