#!/usr/bin/env python3
"""How many slots of the stream layout hold no list entry (CPU only; the pattern comes from the oracle).

k_fill_list's lane = row quad loop evaluates one chain per SLOT of a slice; a dense evaluation would run one chain per
list ENTRY.  For the config-3 problems (seeds 3000 ..., n = m = 200, d = 512, semanticgrav) this prints per problem

  entries   list entries: strict upper by position (position = rank by (degree descending, row ascending))
  slots     sum over the slices of 64 x slice width, widths rounded up to whole quads
  thin      share of the (slice, quad) pairs in which fewer than 16 of the 64 lanes have an entry

and the batch totals.  (1 - entries / slots) bounds the share of evaluation chains a dense evaluation can remove.

    python tools/fill_slot_waste.py [--seeds 16] [--json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def layout_counts(rowptr, cols):
    """(entries, slots, quads, thin quads, L) of the stream layout of one strict-upper CSR pattern."""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    deg = np.bincount(rows, minlength=n) + np.bincount(cols, minlength=n)
    order = np.lexsort((np.arange(n), -deg))              # position -> row
    pos = np.empty(n, dtype=np.int64); pos[order] = np.arange(n)
    upper_of = np.minimum(pos[rows], pos[cols])            # the entry is kept by the end with the smaller position
    cnt = np.bincount(upper_of, minlength=n)
    nsl = (n + 63) // 64
    c = np.zeros(nsl * 64, dtype=np.int64); c[:n] = cnt
    c = c.reshape(nsl, 64)
    width = (c.max(axis=1) + 3) & ~3
    quads = thin = 0
    for s in range(nsl):
        nq = int(width[s]) // 4
        have = (c[s][None, :] > 4 * np.arange(nq)[:, None]).sum(axis=1)     # lanes with an entry in slot quad g (unrotated count: the
        quads += nq; thin += int((have < 16).sum())                          # rotation moves a row's quads around, not their number)
    return int(cnt.sum()), int(64 * width.sum()), quads, thin, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--m", type=int, default=200)
    ap.add_argument("--d", type=int, default=512)
    ap.add_argument("--method", default="semanticgrav")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    from oracle import oracle as orc
    from roman_amd import synth
    from roman_amd.align import SubmapAlignParams
    reg = SubmapAlignParams(method=a.method, semantics_dim=a.d).get_object_registration()
    P = reg._abi_params()
    out = []
    for k in range(a.seeds):
        pr = synth.make_pair(a.n, a.m, a.d, 3000 + k)
        D1, D2 = reg.pack(pr.map1), reg.pack(pr.map2)
        mat, _ = orc.build_matrix(P, D1, D2, reg._association_list(pr.map1, pr.map2))
        rp, cc, _, _ = mat.export()
        e, s, q, t, n = layout_counts(rp, cc)
        out.append({"seed": 3000 + k, "rows": n, "entries": e, "slots": s, "entries_per_slot": round(e / max(s, 1), 4),
                    "quads": q, "thin_quad_share": round(t / max(q, 1), 4)})
        if not a.json:
            print(f"seed {3000 + k}: rows {n:5d}  entries {e:7d}  slots {s:7d}  entries/slots {e / max(s, 1):.3f}  "
                  f"quads {q:4d}  thin (<16 lanes) {t / max(q, 1):.3f}")
    E = sum(r["entries"] for r in out); S = sum(r["slots"] for r in out)
    Q = sum(r["quads"] for r in out); T = sum(r["thin_quad_share"] * r["quads"] for r in out)
    tot = {"problems": len(out), "entries": E, "slots": S, "entries_per_slot": round(E / S, 4), "slot_excess": round(S / E - 1, 4),
           "chains_removable": round(1 - E / S, 4), "thin_quad_share": round(T / Q, 4)}
    if a.json:
        print(json.dumps({"problems": out, "total": tot}))
    else:
        print("total:", json.dumps(tot))


if __name__ == "__main__":
    main()
