"""Particle steering restated in numpy float64, with no engine: what csrc/particles.hip and the host code around it are compared against.

The batch is G groups of K particles, item g K + k being particle k of group g.  Everything here works on (G, K) arrays, so one call serves
every group at once; the sums of a group run in index order (np.cumsum accumulates sequentially, unlike np.sum), as the kernel's do.

    state = new_state(G, K)
    out = particle_weights(state, r, lam, tau, u, final)        # r (G, K) rewards, u (G, 2) uniforms in [0, 1), final (G,) bool: t == 0
    x = gather(x, out["ancestors"])                              # item i takes the content of item ancestors[i]
"""
import numpy as np


def new_state(G, K):
    """logw and rprev start at 0; the counters at 0."""
    return {"logw": np.zeros((G, K)), "rprev": np.zeros((G, K)), "resamples": np.zeros(G, np.int64), "degenerate": np.zeros(G, np.int64)}


def particle_weights(state, r, lam, tau, u, final):
    """One weight update, in place on `state` -> dict ancestors (G*K,) int32 batch indices (identity where nothing was resampled), chosen
    (G,) int32 (the particle picked at t == 0, -1 elsewhere), ess (G,), p (G, K) and c (G, K) (the normalised weights and their running sum,
    for a test's own conditions), resampled (G,) bool.

      1. logw_k += lam (r_k - rprev_k), rprev_k = r_k; a reward or a log-weight of -inf keeps the particle at -inf.
         m = max_k logw_k; p_k = exp(logw_k - m) / sum_j exp(logw_j - m); ESS = 1 / sum_k p_k^2.
      2. All logw_k of the group bit-equal: nothing else happens.
      3. Else if ESS < tau K (and not final): c_k = sum_{j<=k} p_j, with c_k = 1 from the last k with p_k > 0 on (this includes c_{K-1} = 1, and
         keeps a rounding of the sum from handing a threshold to a particle of weight 0); a_i = min{k : c_k > (u + i) / K}, or that last k
         when (u + i) / K rounds to 1; rprev_i = rprev_{a_i}, logw_i = 0, the resample counter goes up.
      4. final: chosen = min{k : c_k > u2}, nothing is resampled.
    A group whose logw are all -inf: left as it is (identity, ESS 0, chosen 0 when final), its degenerate counter goes up."""
    r = np.asarray(r, np.float64)
    G, K = r.shape
    u = np.asarray(u, np.float64).reshape(G, 2)
    final = np.broadcast_to(np.asarray(final, bool), (G,))
    logw, rprev = state["logw"], state["rprev"]
    dead = np.isneginf(r) | np.isneginf(logw)
    with np.errstate(invalid="ignore"):
        inc = lam * (r - rprev)
    logw[...] = np.where(dead, -np.inf, logw + np.where(dead, 0.0, inc))
    rprev[...] = r
    m = logw.max(axis=1)
    degen = np.isneginf(m)
    state["degenerate"] += degen
    equal = (logw.view(np.int64) == logw.view(np.int64)[:, :1]).all(axis=1)
    with np.errstate(invalid="ignore"):
        e = np.exp(logw - np.where(degen, 0.0, m)[:, None])
    e[degen] = 1.0                                                  # (placeholders: the group's outputs are overwritten below)
    tot = np.cumsum(e, axis=1)[:, -1]
    p = e / tot[:, None]
    ess = 1.0 / np.cumsum(p * p, axis=1)[:, -1]
    last = K - 1 - np.argmax(p[:, ::-1] > 0, axis=1)
    c = np.cumsum(p, axis=1)
    c[np.arange(K)[None, :] >= last[:, None]] = 1.0
    resample = ~degen & ~equal & ~final & (ess < tau * K)
    anc = np.tile(np.arange(K), (G, 1))
    rs = np.nonzero(resample)[0]
    if rs.size:
        thr = (u[rs, :1] + np.arange(K)[None, :]) / K               # (groups that resample, K)
        above = c[rs][:, None, :] > thr[:, :, None]                 # (group, i, k)
        anc[rs] = np.where(above.any(axis=2), np.argmax(above, axis=2), last[rs][:, None])
    rows = np.arange(G)[:, None]
    rprev[...] = rprev[rows, anc]
    logw[resample] = 0.0
    state["resamples"] += resample
    pick = c > u[:, 1:2]
    chosen = np.where(pick.any(axis=1), np.argmax(pick, axis=1), last)
    chosen = np.where(final, np.where(degen, 0, chosen), -1)
    ess = np.where(degen, 0.0, ess)
    return {"ancestors": (rows * K + anc).reshape(-1).astype(np.int32), "chosen": chosen.astype(np.int32), "ess": ess, "p": p, "c": c,
            "resampled": resample}


def philox_uniforms(seed, offset, G):
    """(G, 2): group g's (u, u2) as the kernel draws them -- words 0, 1 and 2, 3 of Philox block (seed, offset + g), 27 bits of the first
    above 26 of the second, times 2^-53."""
    from step_nll_restated import philox_words
    w = philox_words(seed, offset, 4 * np.arange(G, dtype=np.uint64)).astype(np.uint64)
    half = lambda hi, lo: (((hi >> np.uint64(5)) << np.uint64(26)) | (lo >> np.uint64(6))).astype(np.float64) * 2.0 ** -53    # noqa: E731
    return np.stack([half(w[0], w[1]), half(w[2], w[3])], axis=1)


def gather(x, ancestors):
    """Item i of x takes the content of item ancestors[i] (out of place: any map, cycles included)."""
    return np.asarray(x)[np.asarray(ancestors)]


def reward_from_partials(part, sigma_y):
    """The built-in reward from the residual pass's fp64 partial sums (B, nblk): folded in index order, r = -(sum / (2 sigma_y^2))."""
    part = np.asarray(part, np.float64)
    return -(np.cumsum(part, axis=1)[:, -1] * (1.0 / (2.0 * sigma_y * sigma_y)))


def measure(video, scale, gray):
    """The cell-mean operators in float64: video (B, T, 3, H, W) -> (B, T, Cy, H / scale, W / scale)."""
    v = np.asarray(video, np.float64)
    B, T, _, H, W = v.shape
    v = v.reshape(B, T, 3, H // scale, scale, W // scale, scale)
    return v.mean(axis=(2, 4, 6))[:, :, None] if gray else v.mean(axis=(4, 6))


def measurement_reward(x0, y, scale, gray, latent, sigma_y):
    """r_b = -rho_b^2 / (2 sigma_y^2), rho_b^2 the sum over the cells of item b's frames with latent == 1 of (y - A x0)^2."""
    res = (np.asarray(y, np.float64) - measure(x0, scale, gray)) ** 2
    lat = np.asarray(latent, np.float64).reshape(res.shape[0], res.shape[1]) == 1.0
    return -(res.sum(axis=(2, 3, 4)) * lat).sum(axis=1) / (2.0 * sigma_y * sigma_y)


# ---- the Gaussian check: one-dimensional data x ~ N(0, prior_std^2) with its exact denoiser, measured as y = x + sigma_w n

def spaced_schedule(steps=50, base=1000):
    """`steps` of `base` linear-beta steps, evenly strided from 0 (the 'ddimN' respacing): the respaced alphas_cumprod."""
    betas = np.linspace(1e-4, 0.02, base, dtype=np.float64)
    acp = np.cumprod(1.0 - betas)
    return acp[::base // steps][:steps]


def gaussian_chain(y, K, rng, prior_std=0.5, sigma_w=0.5, lam=1.0, tau=0.5, steps=50):
    """p_sample (fixed large variance) of the exact denoiser of N(0, prior_std^2) from x_T ~ N(0, 1), K particles for every measurement in
    y (G,), steered by r(x0) = -(y - x0)^2 / (2 sigma_w^2) on the step's x_0 prediction (on the sample itself at t == 0)
    -> (the chosen particle's x_0 per group (G,), the state).  K = 1 is the plain chain."""
    y = np.asarray(y, np.float64)
    G = y.shape[0]
    acp = spaced_schedule(steps)
    acp_prev = np.append(1.0, acp[:-1])
    betas = 1.0 - acp / acp_prev
    coef1 = betas * np.sqrt(acp_prev) / (1.0 - acp)
    coef2 = (1.0 - acp_prev) * np.sqrt(1.0 - betas) / (1.0 - acp)
    post_var = betas * (1.0 - acp_prev) / (1.0 - acp)
    var = np.append(post_var[1], betas[1:])
    v = prior_std ** 2
    x = rng.standard_normal((G, K))
    state = new_state(G, K)
    out = None
    for t in range(steps - 1, -1, -1):
        x0 = x * np.sqrt(acp[t]) * v / (acp[t] * v + 1.0 - acp[t])
        x = coef1[t] * x0 + coef2[t] * x + (np.sqrt(var[t]) * rng.standard_normal((G, K)) if t > 0 else 0.0)
        if K > 1:
            r = -((y[:, None] - (x if t == 0 else x0)) ** 2) / (2.0 * sigma_w ** 2)
            out = particle_weights(state, r, lam, tau, rng.random((G, 2)), t == 0)
            x = gather(x.reshape(-1), out["ancestors"]).reshape(G, K)
    chosen = out["chosen"] if K > 1 else np.zeros(G, np.int64)
    return x[np.arange(G), chosen], state


def ddnm_plus_chain(y, rng, prior_std=0.5, sigma_w=0.5, steps=50):
    """The alternative that stays out, on the same one-dimensional model: DDNM+'s scaled correction (Wang, Yu, Zhang 2022, eq.
    19) for A = I -- x0' = x0 + l_t (y - x0) with l_t = min(1, s_t / (a_t sigma_w)), a_t the posterior mean's coefficient of x0 and
    s_t^2 the step's variance, and the noise reduced to s_t^2 - (a_t l_t sigma_w)^2 -> the samples (G,)."""
    y = np.asarray(y, np.float64)
    acp = spaced_schedule(steps)
    acp_prev = np.append(1.0, acp[:-1])
    betas = 1.0 - acp / acp_prev
    coef1 = betas * np.sqrt(acp_prev) / (1.0 - acp)
    coef2 = (1.0 - acp_prev) * np.sqrt(1.0 - betas) / (1.0 - acp)
    var = np.append((betas * (1.0 - acp_prev) / (1.0 - acp))[1], betas[1:])
    v = prior_std ** 2
    x = rng.standard_normal(y.shape[0])
    for t in range(steps - 1, -1, -1):
        x0 = x * np.sqrt(acp[t]) * v / (acp[t] * v + 1.0 - acp[t])
        s = np.sqrt(var[t]) if t > 0 else 0.0
        lam = min(1.0, s / (coef1[t] * sigma_w))
        x0 = x0 + lam * (y - x0)
        x = coef1[t] * x0 + coef2[t] * x + np.sqrt(max(s * s - (coef1[t] * lam * sigma_w) ** 2, 0.0)) * rng.standard_normal(y.shape[0])
    return x
