"""Shared pieces of the per-atom virial tests (TEST INFRASTRUCTURE): the
edge-gradient partition written out in fp64 numpy, and the error bounds the
tests hold the device result to.

Definition ("Per-atom virial"): edge e = (centre i, neighbour j)
with r = edge_vec and g = dE/dr has the virial term

    v_e = -(r_x g_x, r_y g_y, r_z g_z, (r_x g_y + r_y g_x)/2,
            (r_y g_z + r_z g_y)/2, (r_x g_z + r_z g_x)/2)

(library order xx yy zz xy yz zx), and W_a = 1/2 sum_{centre(e)=a} v_e +
1/2 sum_{nbr(e)=a} v_e.
"""
import numpy as np

U = 2.0 ** -24            # fp32 unit roundoff
PAIRS = [(0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2)]


def edge_terms(vec, grad):
    """(v [E, 6], a [E, 6]): the edges' virial terms in fp64, and the same with
    every product replaced by its absolute value (what a rounding-error bound
    of the products and their sum is proportional to)."""
    r, g = np.asarray(vec, dtype=np.float64), np.asarray(grad, dtype=np.float64)
    v, a = np.empty((len(r), 6)), np.empty((len(r), 6))
    for q, (i, j) in enumerate(PAIRS):
        if i == j:
            v[:, q] = -r[:, i] * g[:, i]
            a[:, q] = np.abs(r[:, i] * g[:, i])
        else:
            v[:, q] = -0.5 * (r[:, i] * g[:, j] + r[:, j] * g[:, i])
            a[:, q] = 0.5 * (np.abs(r[:, i] * g[:, j]) + np.abs(r[:, j] * g[:, i]))
    return v, a


def _ends(n, center, nbr, x, sides=(True, True)):
    out = np.zeros((n,) + x.shape[1:])
    if sides[0]:
        np.add.at(out, np.asarray(center, dtype=np.int64), x)
    if sides[1]:
        np.add.at(out, np.asarray(nbr, dtype=np.int64), x)
    return out


def partition(n, center, nbr, vec, grad, sides=(True, True)):
    """fp64 partition of the given edge vectors and gradients.  Returns
    (W [n, 6], S [n, 6], m [n]): S the sum of the absolute values of the terms
    of every entry (each product of r and g, halved as in W), m the number of
    edge ends on the atom.  ``sides``: (centre side, neighbour side)."""
    v, a = edge_terms(vec, grad)
    W = _ends(n, center, nbr, 0.5 * v, sides)
    S = _ends(n, center, nbr, 0.5 * a, sides)
    m = _ends(n, center, nbr, np.ones(len(v)), sides)
    return W, S, m


def kernel_bound(S, m):
    """T1: (m_a + 4) u S_aq -- the recursive-summation bound of an fp32 sum of
    m_a terms (m_a - 1 roundings), each a product or a sum of two products
    scaled by a power of two (at most three roundings)."""
    return (m[:, None] + 4) * U * S


def sum_bound(vec, grad):
    """T2: (E + 4) u sum_e |terms| per Voigt entry, for sum_a W_a against the
    library's virial6 (an fp32 tree sum of the same E terms)."""
    _, a = edge_terms(vec, grad)
    return (len(a) + 4) * U * a.sum(0)


def gradient_bound(n, center, nbr, vec, grad, f_tol):
    """The T3 form: what a per-edge gradient error of ``f_tol`` (eV/A, per
    component) and the fp32 rounding of the edge vectors can move an entry by,
    f_tol * 1/2 sum_ends w_q(r_e) + sum_ends u |r_e| |g_e|, with w_q = |r_a| on
    the diagonal and (|r_a| + |r_b|) / 2 off it.  The kernel bound comes on top."""
    r, g = np.abs(np.asarray(vec, dtype=np.float64)), np.asarray(grad, dtype=np.float64)
    w = np.stack([r[:, i] if i == j else 0.5 * (r[:, i] + r[:, j]) for i, j in PAIRS], axis=1)
    rg = np.linalg.norm(vec, axis=1) * np.linalg.norm(g, axis=1)
    return f_tol * _ends(n, center, nbr, 0.5 * w) + U * _ends(n, center, nbr, rg)[:, None]
