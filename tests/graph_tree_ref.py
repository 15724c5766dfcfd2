"""The tree preconditioner of DESIGN.md 4.17 restated in numpy over graph_ref: the spanning-forest rule, M assembled densely, the block
factorisation and its two sweeps node by node, and the preconditioned conjugate gradient as the solve kernel runs it.

Written independently of csrc/graph_forest.h: components are label lists merged in place, parents come from a depth-first walk, and the
elimination order is that walk's post-order (any order with children before parents gives the same factors up to rounding)."""
import numpy as np

BLOCK_JACOBI, TREE = 0, 1


def forest(n, edges, prior_ids):
    """The rule: the between factors in the order added; one joins the forest when its ends lie in different components; every other one is a
    loop for the preconditioner.  The root of a component is its lowest-numbered pose that holds a prior.
    edges: [(from, to)]; -> dict(parent (n,), in_tree [bool], tree_factor (n,), n_tree, n_other, order (children before parents))"""
    label = list(range(n))
    members = {p: [p] for p in range(n)}
    in_tree = []
    adj = [[] for _ in range(n)]
    for e, (i, j) in enumerate(edges):
        a, b = label[i], label[j]
        if a == b:
            in_tree.append(False)
            continue
        in_tree.append(True)
        adj[i].append((j, e))
        adj[j].append((i, e))
        if len(members[a]) < len(members[b]):
            a, b = b, a
        for p in members[b]:
            label[p] = a
        members[a] += members.pop(b)
    with_prior = set(int(k) for k in prior_ids)
    parent = np.full(n, -1, dtype=np.int64)
    tree_factor = np.full(n, -1, dtype=np.int64)
    order = []
    for comp in members.values():
        held = sorted(p for p in comp if p in with_prior)
        root = held[0] if held else min(comp)
        stack, seen = [(root, iter(adj[root]))], {root}
        while stack:
            p, it = stack[-1]
            for q, e in it:
                if q not in seen:
                    seen.add(q)
                    parent[q], tree_factor[q] = p, e
                    stack.append((q, iter(adj[q])))
                    break
            else:
                order.append(p)
                stack.pop()
    return dict(parent=parent, in_tree=in_tree, tree_factor=tree_factor, n_tree=sum(in_tree), n_other=len(in_tree) - sum(in_tree), order=order)


def graph_forest(g):
    return forest(len(g.poses), [(i, j) for i, j, _, _ in g.betweens], [k for k, _, _ in g.priors])


def dense_m(g, lam, kind=TREE, fr=None):
    """M (6N, 6N): lam I + every prior + the forest's between factors (TREE), or the diagonal blocks of H + lam I (BLOCK_JACOBI)"""
    n = len(g.poses)
    if kind == BLOCK_JACOBI:
        H, _, _ = g.normal_equations()
        M = np.zeros_like(H)
        for p in range(n):
            s = slice(6 * p, 6 * p + 6)
            M[s, s] = H[s, s]
        return M + lam * np.eye(6 * n)
    fr = fr or graph_forest(g)
    _, jf, jt, _ = g.linearize()
    M = lam * np.eye(6 * n)
    for e, (k, _P, Om) in enumerate(g.priors):
        s = slice(6 * k, 6 * k + 6)
        M[s, s] += jt[e].T @ Om @ jt[e]
    for e, (i, j, _Z, Om) in enumerate(g.betweens):
        if not fr["in_tree"][e]:
            continue
        a, b = jf[len(g.priors) + e], jt[len(g.priors) + e]
        si, sj = slice(6 * i, 6 * i + 6), slice(6 * j, 6 * j + 6)
        M[si, si] += a.T @ Om @ a
        M[sj, sj] += b.T @ Om @ b
        M[si, sj] += a.T @ Om @ b
        M[sj, si] += b.T @ Om @ a
    return M


class TreeFactor:
    """Block Cholesky of M from the leaves to the roots (no fill on a forest), node by node:
    D_p = A_pp - sum over children G_c A_cp,  G_c = A_pc D_c^-1;  forward y_p = r_p - sum G_c y_c;  backward z_p = D_p^-1 y_p - G_p^T z_parent."""

    def __init__(self, g, lam, fr=None):
        self.n = len(g.poses)
        self.fr = fr or graph_forest(g)
        M = dense_m(g, lam, TREE, self.fr)
        n, parent = self.n, self.fr["parent"]
        blk = lambda a, b: M[6 * a:6 * a + 6, 6 * b:6 * b + 6]
        self.D = [blk(p, p).copy() for p in range(n)]
        self.G = [None] * n
        self.ok = True
        for c in self.fr["order"]:
            try:
                np.linalg.cholesky(self.D[c])
            except np.linalg.LinAlgError:
                self.ok = False
            p = parent[c]
            if p < 0:
                continue
            A_pc = blk(p, c)
            self.G[c] = np.linalg.solve(self.D[c], A_pc.T).T          # A_pc D_c^-1 (D symmetric)
            self.D[p] = self.D[p] - self.G[c] @ A_pc.T

    def solve(self, r):
        parent, order = self.fr["parent"], self.fr["order"]
        y = np.asarray(r, dtype=np.float64).reshape(self.n, 6).copy()
        for c in order:
            if parent[c] >= 0:
                y[parent[c]] -= self.G[c] @ y[c]
        z = np.stack([np.linalg.solve(self.D[p], y[p]) for p in range(self.n)]) if self.n else y
        for c in reversed(order):
            if parent[c] >= 0:
                z[c] -= self.G[c].T @ z[parent[c]]
        return z.reshape(-1)


def backward_error(M, z, r):
    """|Mz - r|_inf / (|M|_inf |z|_inf + |r|_inf)"""
    den = np.linalg.norm(M, np.inf) * np.abs(z).max() + np.abs(r).max()
    return float(np.abs(M @ z - r).max() / den) if den > 0 else 0.0


def pcg(H, g, lam, apply_minv, tol=1e-10, max_it=None):
    """(H + lam I) x = -g as graph_solve_kernel runs it: x0 = 0, stop on |res| / |g| <= tol.  -> x, iterations, capped"""
    n = g.size
    max_it = max(100, 10 * (n // 6)) if max_it is None else max_it
    A = H + lam * np.eye(n)
    x = np.zeros(n)
    res = -g
    gnorm = np.linalg.norm(g)
    if gnorm == 0.0:
        return x, 0, False
    z = apply_minv(res)
    d = z.copy()
    rz = res @ z
    it = 0
    while it < max_it:
        ap = A @ d
        alpha = rz / (d @ ap)
        x += alpha * d
        res = res - alpha * ap
        it += 1
        if not np.linalg.norm(res) / gnorm > tol:
            return x, it, False
        z = apply_minv(res)
        nz = res @ z
        d = z + (nz / rz) * d
        rz = nz
    return x, it, True


def minv(g, lam, kind):
    """the preconditioner's action at g's estimates"""
    if kind == TREE:
        return TreeFactor(g, lam).solve
    H, _, _ = g.normal_equations()
    inv = [np.linalg.inv(H[6 * p:6 * p + 6, 6 * p:6 * p + 6] + lam * np.eye(6)) for p in range(len(g.poses))]
    return lambda r: np.concatenate([inv[p] @ r[6 * p:6 * p + 6] for p in range(len(inv))])


def first_solve_iterations(g, kind, lam=1e-5, tol=1e-10):
    """PCG iterations of the first trial step of an optimisation of g (lambda_init, the estimates as they stand)"""
    H, grad, _ = g.normal_equations()
    _, it, capped = pcg(H, grad, lam, minv(g, lam, kind), tol)
    return it, capped
