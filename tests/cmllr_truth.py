"""Truth of the CMLLR statistics, objective, transform and row update: numpy longdouble sums
written from the definitions, with no code of the package.

Every sum comes back with the sum of the absolute values of its terms and the number of terms,
which is what the tests' error bound is made of:  |got - truth| <= (n + 4) 2^-52 sum |terms|.

    r_tk     = comp_resps[t, k] * state_resps[t, k // G]
    omega_ti = sum_k r_tk E[lambda]_ki      (P columns: D diagonal, 1 isotropic)
    nu_ti    = sum_k r_tk E[lambda mu]_ki
    c_t      = sum_k r_tk
    G_{s,i}  = sum_t omega_ti xi_t xi_t^T,  k_{s,i} = sum_t nu_ti xi_t,  beta_s = sum_t c_t
    Q_s(W)   = beta ln|det A| + sum_i (w_i . k_i - 1/2 w_i G_i w_i^T)
"""

import numpy as np

LD = np.longdouble


def frame_params(comp_resps, state_resps, E, S, G, D, P):
    '''(value, abs, n) of [omega | nu | c], [T, P + D + 1] longdouble; `E` [S G, Q] holds
    E[lambda mu] in its first D columns and E[lambda] in the next P.'''
    K = S * G
    T = len(comp_resps) if comp_resps is not None else len(state_resps)
    value = np.zeros((T, P + D + 1), dtype=LD)
    mag = np.zeros_like(value)
    E = np.asarray(E, dtype=LD)
    for k in range(K):
        r = np.ones(T, dtype=LD)
        if comp_resps is not None:
            r = r * np.asarray(comp_resps[:, k], dtype=LD)
        if state_resps is not None:
            r = r * np.asarray(state_resps[:, k // G], dtype=LD)
        row = np.concatenate([E[k, D:D + P], E[k, :D], np.ones(1, dtype=LD)])
        term = r[:, None] * row[None, :]
        value += term
        mag += np.abs(term)
    return value, mag, K


def extended(X):
    X = np.asarray(X, dtype=LD)
    return np.concatenate([X, np.ones((len(X), 1), dtype=LD)], axis=1)


def statistics(X, params, lengths, speakers, n_spk, P):
    '''(G, k, beta), each a (value, abs, n) triple: G [n_spk, P, E, E] as full symmetric
    matrices, k [n_spk, D, E], beta [n_spk]; n [n_spk] the frames of every speaker.'''
    X = np.asarray(X, dtype=LD)
    T, D = X.shape
    E = D + 1
    xi = extended(X)
    prm = np.asarray(params, dtype=LD)
    om, nu, c = prm[:, :P], prm[:, P:P + D], prm[:, P + D]
    Gv, Ga = np.zeros((n_spk, P, E, E), dtype=LD), np.zeros((n_spk, P, E, E), dtype=LD)
    kv, ka = np.zeros((n_spk, D, E), dtype=LD), np.zeros((n_spk, D, E), dtype=LD)
    bv, ba = np.zeros(n_spk, dtype=LD), np.zeros(n_spk, dtype=LD)
    n = np.zeros(n_spk, dtype=np.int64)
    t0 = 0
    for length, s in zip(lengths, speakers):
        t1 = t0 + length
        if s >= 0 and length:
            # (|omega xi_a xi_b| = |omega| |xi_a| |xi_b|: the absolute sums are the same sums of
            #  the absolute factors; einsum on longdouble is a plain loop, frame after frame)
            x, o, v = xi[t0:t1], om[t0:t1], nu[t0:t1]
            outer = x[:, :, None] * x[:, None, :]
            Gv[s] += np.einsum('ti,tab->iab', o, outer)
            Ga[s] += np.einsum('ti,tab->iab', np.abs(o), np.abs(outer))
            kv[s] += np.einsum('ti,ta->ia', v, x)
            ka[s] += np.einsum('ti,ta->ia', np.abs(v), np.abs(x))
            bv[s] += c[t0:t1].sum()
            ba[s] += np.abs(c[t0:t1]).sum()
            n[s] += length
        t0 = t1
    return (Gv, Ga, n), (kv, ka, n), (bv, ba, n)


def pack_lower(Gfull):
    'The packed lower triangles [..., E (E + 1) / 2] of [..., E, E], row by row.'
    E = Gfull.shape[-1]
    a, b = np.tril_indices(E)
    return Gfull[..., a, b]


def log_abs_det(A):
    'ln|det A| in longdouble: Gaussian elimination with partial pivoting.'
    A = np.array(A, dtype=LD)
    n = len(A)
    total = LD(0)
    for j in range(n):
        p = j + int(np.argmax(np.abs(A[j:, j])))
        if A[p, j] == 0:
            return -np.inf
        if p != j:
            A[[j, p]] = A[[p, j]]
        total += np.log(np.abs(A[j, j]))
        A[j + 1:] -= (A[j + 1:, j] / A[j, j])[:, None] * A[j][None, :]
    return total


def objective_from_stats(W, Gfull, k, beta):
    'Q(W) of ONE speaker from its statistics: Gfull [P, E, E], k [D, E], beta.'
    W = np.asarray(W, dtype=LD)
    D = len(W)
    q = LD(beta) * log_abs_det(W[:, :D]) if beta != 0 else LD(0)
    for i in range(D):
        Gi = Gfull[i if len(Gfull) > 1 else 0]
        q += W[i] @ k[i] - LD(.5) * (W[i] @ Gi @ W[i])
    return q


def objective_from_frames(W, X, params, P):
    'Q(W) of ONE speaker directly from its frames: sum_t c_t ln|det A| + nu . y - omega . y^2 / 2.'
    W = np.asarray(W, dtype=LD)
    D = len(W)
    y = extended(X) @ W.T
    prm = np.asarray(params, dtype=LD)
    om, nu, c = prm[:, :P], prm[:, P:P + D], prm[:, P + D]
    beta = c.sum()
    q = beta * log_abs_det(W[:, :D]) if beta != 0 else LD(0)
    return q + (nu * y).sum() - LD(.5) * (om * y * y).sum()


def apply(X, W, lengths, speakers):
    '(value, abs, n) of Y[t] = A_s x_t + b_s, longdouble; speaker -1 copies (abs = |x|, n = 1).'
    X = np.asarray(X, dtype=LD)
    D = X.shape[1]
    value, mag = X.copy(), np.abs(X)
    n = np.ones(len(X), dtype=np.int64)
    xi = extended(X)
    t0 = 0
    for length, s in zip(lengths, speakers):
        t1 = t0 + length
        if s >= 0:
            Ws = np.asarray(W[s], dtype=LD)
            for t in range(t0, t1):
                term = Ws * xi[t][None, :]
                value[t] = term.sum(axis=1)
                mag[t] = np.abs(term).sum(axis=1)
            n[t0:t1] = D + 1
        t0 = t1
    return value, mag, n


def row_update(W, Gfull, k, beta, i):
    '''The row update of ONE speaker, restated in float64 from Gales (1998): p = [cof_i(A), 0]
    with the cofactors det(A) A^-T[i]; a = p G_i^-1 p^T, b = p G_i^-1 k_i; the root alpha of
    a alpha^2 + b alpha - beta = 0 with the larger beta ln|alpha a + b| - alpha^2 a / 2;
    w_i = (alpha p + k_i) G_i^-1.  Returns the new W.'''
    W = np.array(W, dtype=np.float64)
    D = len(W)
    A = W[:, :D]
    cof = np.linalg.det(A) * np.linalg.inv(A).T[i]
    p = np.concatenate([cof, [0.]])
    Ginv = np.linalg.inv(np.asarray(Gfull[i if len(Gfull) > 1 else 0], dtype=np.float64))
    ki = np.asarray(k[i], dtype=np.float64)
    a, b = p @ Ginv @ p, p @ Ginv @ ki
    best = None
    for sign in (1., -1.):
        alpha = (-b + sign * np.sqrt(b * b + 4. * a * float(beta))) / (2. * a)
        value = float(beta) * np.log(abs(alpha * a + b)) - .5 * alpha * alpha * a
        if best is None or value > best[0]:
            best = (value, alpha)
    W[i] = (best[1] * p + ki) @ Ginv
    return W
