"""The reference's mno_clipper loop [REF roman/align/object_registration.py:57-86] on the CPU oracle: dense M and C of the scored
pair, then `K` plain-CLIPPER solves (invariant = ROMAN_INV_EUCLIDEAN: strict upper triangles, implicit identity diagonal, u0 = 1)
with the selected block of M zeroed between them — composed exactly as tests/test_gpu_batch.py::test_dense_matrix_path_and_mno_clipper."""
import numpy as np

from roman_amd import _abi


def plain_params(reg):
    P = _abi.RomanParams.from_buffer_copy(reg._abi_params())
    P.invariant = _abi.ROMAN_INV_EUCLIDEAN
    return P


def mno_from_dense(orc, P, Mo, Co, A, K, mask_c=False):
    """-> list of dict(assoc int64 (k,2), nodes, score, stats).  mask_c=True is the OTHER reading of the masking step (the pair
    is removed from C as well), used only to show that a test problem tells the two apart."""
    Mw, Cw = Mo.copy(), Co.copy()
    out = []
    for k in range(K):
        s = orc.solve(P, orc.matrix_from_dense(Mw, Cw))
        nodes = s["nodes"]
        u_sol = np.zeros_like(s["u"]); u_sol[nodes] = s["u"][nodes]
        score = 0.0 if len(nodes) == 0 else float(u_sol @ Mo @ u_sol / (u_sol @ u_sol))
        out.append(dict(assoc=np.asarray(A)[nodes].astype(np.int64).reshape(len(nodes), 2), nodes=nodes.copy(), score=score, stats=s["stats"]))
        if k + 1 < K and len(nodes):
            Mw[np.ix_(nodes, nodes)] = 0.0
            if mask_c:
                Cw[np.ix_(nodes, nodes)] = 0.0; Cw[nodes, nodes] = 1.0
    return out


def oracle_mno(orc, reg, m1, m2, K):
    D1, D2 = reg.pack(m1), reg.pack(m2)
    mat, A = orc.build_matrix(reg._abi_params(), D1, D2, reg._association_list(m1, m2))
    Mo, Co = mat.dense()
    return mno_from_dense(orc, plain_params(reg), Mo, Co, A, K)


def pose_of(orc, m1, m2, assoc, dim=3):
    p1 = np.array([m1[i].center.ravel()[:dim] for i, _ in assoc]); p2 = np.array([m2[j].center.ravel()[:dim] for _, j in assoc])
    return orc.t_align(p1, p2, dim)
