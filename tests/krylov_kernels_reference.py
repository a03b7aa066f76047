"""What each launch wrapper of the Krylov step's reductions and vector updates must return: a numpy + math.fsum
restatement written from the comments above the kernels of fedm_amd/csrc/kernels.hip and the second half of spmv.hip
(helper module; tests/test_krylov_kernels_reference.py pins it, tests/test_gpu_krylov_kernels.py holds the device to it).

Vectors are the device's: ``np_`` entries, of which the first ``n_dot`` take part in reductions (the owned rows); what
lies behind them -- ghost rows on a rank, then the padding rows -- holds a sentinel (:func:`padded`).  Sums are exact
(fsum of the float64 products) over the first n_dot entries only, weighted by ``wgt`` where given; with each sum comes
sum |terms|, which the bounds are stated in.  Updates are done entry by entry over all np_ entries in the kernel's
order: chunks of eight vectors, the scale in the last chunk only.

``perturb`` names one deliberate fault (PERTURBATIONS): a kernel with that fault must miss the bound by more than 100x,
which the CPU test asserts of the restatement -- the convention of fieldsplit_reference.PERTURBATIONS."""
import math

import numpy as np

RED_K, RED_BLOCKS = 40, 512
RED_SPARE, RED_REFINE = RED_K - 3, RED_K - 4
VEC_BLOCKS = 2048                     # vec_grid's cap
EPS = float(np.finfo(np.float64).eps)
FIELD_EPS = 3.0e-16                   # DOLFIN_EPS of field_error_kernel

PERTURBATIONS = ("last", "range", "swap8", "chunk_base", "final_every_chunk", "self", "stride")


def padded(v, n_dot, np_, sentinel=1e30):
    """The device's copy of a caller's vector: its first n_dot entries, the sentinel behind them."""
    out = np.full(np_, sentinel)
    out[:n_dot] = np.asarray(v, dtype=np.float64).reshape(-1)[:n_dot]
    return out


def _exact(terms):
    return math.fsum(terms.tolist()), math.fsum(np.abs(terms).tolist())


def _range(n_dot, np_, perturb, blocks=RED_BLOCKS):
    """The entries a reduction visits."""
    if perturb == "last":
        return slice(0, n_dot - 1)
    if perturb == "range":
        return slice(0, np_)
    if perturb == "stride":          # the grid-stride loop stopped after its first trip
        grid = min((n_dot + 255) // 256, blocks)
        return slice(0, min(n_dot, grid * 256))
    return slice(0, n_dot)


def dots(V, y, n_dot, k, wgt=None, perturb=None):
    """(sums, sum |terms|) of V[i] . y, i < k -- dots_kernel, launch_dots' chunks of eight."""
    y = np.asarray(y)
    r = _range(n_dot, y.size, perturb)
    yw = y[r] * wgt[r] if wgt is not None else y[r]
    s, a = np.zeros(k), np.zeros(k)
    for i in range(k):
        s[i], a[i] = _exact(np.asarray(V[i])[r] * yw)
    if perturb == "chunk_base":      # every chunk writes from slot 0: the last chunk's sums win, slots 8 and up stay 0
        out, oa = np.zeros(k), np.zeros(k)
        for i in range(k):
            out[i % 8], oa[i % 8] = s[i], a[i]
        return out, oa
    return s, a


def dots_fused(V, y, n_dot, k, neq, x0=None, y_index=-1, wgt=None, perturb=None):
    """dots_scatter_kernel: the potential component of y is taken from x0 first (the owned vertices), then V[i] . y with
    the NEW y wherever V[i] is y itself.  Returns (sums, sum |terms|, y as left)."""
    y = np.array(V[y_index] if y_index >= 0 else y, dtype=np.float64)
    old = y.copy()
    if x0 is not None:
        nvert = n_dot // neq
        y[neq - 1:nvert * neq:neq] = np.asarray(x0)[:nvert]
    # launch_dots_fused hands x0 to the first chunk only: in a later chunk y's potential component is the stored one,
    # which is the same values
    W = [np.asarray(v) for v in V[:k]]
    if y_index >= 0 and y_index < k:
        W[y_index] = old if perturb == "self" else y
    s, a = dots(W, y, n_dot, k, wgt=wgt, perturb=None if perturb == "self" else perturb)
    return s, a, y


def norm2(x, n_dot, wgt=None, perturb=None):
    s, a = dots([x], x, n_dot, 1, wgt=wgt, perturb=perturb)
    return s[0], a[0]


def finish_values(h, ww):
    """The finish formulae on given sums: (hn2, sound, scale) -- Pythagoras with V orthonormal, hn2 = ww - sum h_i^2
    summed in the slots' order, trusted when hn2 > 1e-8 ww and hn2 > 0."""
    hh = 0.0
    for v in h:
        hh += float(v) * float(v)
    hn2 = float(ww) - hh
    sound = hn2 > 1e-8 * float(ww) and hn2 > 0.0
    return hn2, sound, (1.0 / math.sqrt(hn2) if sound else 1.0)


def finish(sums, k, red_before, kind, flag_refine=False):
    """Row 0 of the reduction buffer after a finish on ``sums`` (k slots: h_0 .. h_{k-2}, ww).
    kind "cgs" (cgs_finish_kernel, launch_dots): in place, every other slot keeps what it held.
    kind "reduce" (reduce_finish_kernel, spmv_dots_finish_kernel): every other slot 0, RED_SPARE carried through;
    flag_refine (finish = 2): RED_REFINE = 0 when sound, 1 when not."""
    red_before = np.asarray(red_before, dtype=np.float64)
    if kind == "cgs":
        out = red_before.copy()
    else:
        out = np.zeros(RED_K)
        out[RED_SPARE] = red_before[RED_SPARE]
    out[:k] = sums[:k]
    hn2, sound, scale = finish_values(sums[:k - 1], sums[k - 1])
    out[RED_K - 2] = sums[k - 1]
    out[k - 1] = hn2
    out[RED_K - 1] = scale
    if flag_refine:
        out[RED_REFINE] = 0.0 if sound else 1.0
    return out


def cgs_update(y, V, coef, k, final=True, perturb=None):
    """y = (y - sum_i coef[i] V[i]) coef[RED_K-1]: launch_cgs_update's chunks of eight, the scale in the last.
    Returns (y, magnitude) with magnitude = (|y| + sum |c_i x_i|) |scale| per entry, what the bound is stated in."""
    y = np.array(y, dtype=np.float64)
    coef = np.array(coef, dtype=np.float64)
    if perturb == "swap8":
        for i in range(0, k - 8):
            if (i // 8) % 2 == 0:
                coef[i], coef[i + 8] = coef[i + 8], coef[i]
    scale = coef[RED_K - 1] if final else 1.0
    mag = np.abs(y)
    done = 0
    while done < k:
        kk = min(8, k - done)
        base = 0 if perturb == "chunk_base" else done
        for i in range(kk):
            y = y - coef[base + i] * np.asarray(V[done + i])
            mag = mag + np.abs(coef[base + i] * np.asarray(V[done + i]))
        if done + kk == k or perturb == "final_every_chunk":
            y = y * scale
        done += kk
    return y, mag * abs(scale)


def multi_axpy(y, V, coef, k, sign=1.0, perturb=None):
    """y += sign sum_i coef[i] V[i] (launch_multi_axpy; the coefficients travel as sign * coef[i])."""
    y = np.array(y, dtype=np.float64)
    coef = np.array(coef, dtype=np.float64)
    if perturb == "swap8":
        for i in range(0, k - 8):
            if (i // 8) % 2 == 0:
                coef[i], coef[i + 8] = coef[i + 8], coef[i]
    mag = np.abs(y)
    for i in range(k):
        c = sign * coef[(i % 8) if perturb == "chunk_base" else i]
        y = y + c * np.asarray(V[i])
        mag = mag + np.abs(c * np.asarray(V[i]))
    return y, mag


def newton_update(u, Z, coef, k, n_dot, perturb=None):
    """delta = sum_i coef[i] Z[i], u += delta; |delta|^2 and |u|^2 over the first n_dot entries.
    Returns (u, delta, magnitude of u, magnitude of delta, (|delta|^2, sum |terms|), (|u|^2, sum |terms|))."""
    u = np.asarray(u, dtype=np.float64)
    d = np.zeros(u.size)
    mag = np.zeros(u.size)
    for i in range(k):
        d = d + coef[i] * np.asarray(Z[i])
        mag = mag + np.abs(coef[i] * np.asarray(Z[i]))
    un = u + d
    r = _range(n_dot, u.size, perturb)
    return un, d, mag + np.abs(u), mag, _exact(d[r] * d[r]), _exact(un[r] * un[r])


def normalise_copy(x, n2):
    """y = x / sqrt(n2); 0 when that norm is 0, negative, infinite or NaN."""
    a = 1.0 / math.sqrt(n2) if (n2 > 0.0 and n2 < 1.7e308) else 0.0
    return a * np.asarray(x, dtype=np.float64)


def first_stage(t, dinv, nv, ns):
    """g = Duu^-1 t_u rounded to single precision and b0 = t_phi for nv vertices; dinv [nv][ns][ns] in float64.
    Returns (g32 as float64, sum |dinv t| per entry, b0)."""
    T = np.asarray(t)[:nv * (ns + 1)].reshape(nv, ns + 1)
    g = np.einsum("vrc,vc->vr", dinv, T[:, :ns])
    mag = np.einsum("vrc,vc->vr", np.abs(dinv), np.abs(T[:, :ns]))
    return g.astype(np.float32).astype(np.float64), mag, T[:, ns].copy()


def species_block_inverses(J, nv, ns):
    """Duu^-1 per vertex from a CSR Jacobian in the vectors' numbering."""
    neq = ns + 1
    D = np.empty((nv, ns, ns))
    rows = np.arange(nv) * neq
    for r in range(ns):
        for c in range(ns):
            D[:, r, c] = np.asarray(J[rows + r, rows + c]).ravel()
    return np.linalg.inv(D)


def refine(red, V, t, n_dot, k, wgt=None):
    """launch_cgs_refine behind step j = k - 2 on red = the two rows as the first finish left them.  Returns (red rows
    after, t after, magnitude per entry of the update, sums (c_0 .. c_{k-2}, tt), their sum |terms|); with the flag
    at 0 nothing changes and the sums are None."""
    red = np.array(red, dtype=np.float64).reshape(2, RED_K)
    t = np.array(t, dtype=np.float64)
    if red[0, RED_REFINE] == 0.0:
        return red, t, np.abs(t), None, None
    s, a = dots(list(V[:k - 1]) + [t], t, n_dot, k, wgt=wgt)
    hn2, sound, scale = finish_values(s[:k - 1], s[k - 1])
    red[0, :k - 1] += s[:k - 1]
    red[1, :k - 1] = s[:k - 1]
    red[0, k - 1] = hn2
    red[0, RED_K - 1] = red[1, RED_K - 1] = scale
    red[0, RED_REFINE] = 1.0 if sound else 2.0
    t2, mag = cgs_update(t, V, red[1], k - 1)
    return red, t2, mag, s, a


def field_error(u, uold, n_owned, neq, comp):
    """((|new - old + eps|^2, sum |terms|), (|old + eps|^2, sum |terms|)) over one component of the owned vertices."""
    a = np.asarray(u)[comp:n_owned * neq:neq]
    b = np.asarray(uold)[comp:n_owned * neq:neq]
    d, o = a - b + FIELD_EPS, b + FIELD_EPS
    return _exact(d * d), _exact(o * o)


def spmv_dots(J, z, V, n_owned, neq, k, wgt=None):
    """w = J z on the owned rows (0 on the ghost rows), h_i = V[i] . w for i < k - 1 and ww = w . w over them.
    Returns (w, |J| |z| per row, sums, sum |terms|); J: CSR over the n = nv * neq caller entries."""
    n = J.shape[0]
    z = np.asarray(z)[:n]
    w = J @ z
    mag = abs(J) @ np.abs(z)
    n_dot = n_owned * neq
    w[n_dot:] = 0.0
    mag[n_dot:] = 0.0
    s, a = dots([np.asarray(v)[:n] for v in V[:k - 1]] + [w], w, n_dot, k, wgt=wgt)
    return w, mag, s, a
