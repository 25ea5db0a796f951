"""Model of option bin_split from the CPU oracle alone (no GPU): what the fan loops of k_integ / k_fric run and what vertex fields
they read when a chunk's kept polygons are binned by vertex count.

    python scripts/binned_fill_model.py [n_poses] [chunk]

The oracle's candidate list of n_poses full-size C3 poses (debug view: clip_n per candidate, in the oracle's order -- the device's
list is grouped by item in the same way, in another order inside an item) is cut into chunks of `chunk` candidates; the polygons
(clip_n >= 3) of a chunk are laid out densely, or front / back by `n < split`, and walked in 64-slot pieces as kept_slot does
(pfc_np.h: the block both regions end in is walked once).  A piece costs max(n) fan iterations and reads max(n) vertex slots of 64
lanes x 24 bytes, whatever its other lanes hold.  Printed per split: pieces, fan iterations per piece, and both sums against the
dense fill."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def pieces(n, C, split):
    """Lists of vertex counts, one per 64-slot piece of a chunk whose polygons have the vertex counts n (in list order)."""
    if split == 0:
        return [n[p:p + 64] for p in range(0, len(n), 64)]
    slot = np.zeros(C, dtype=int)
    a, b = n[n < split], n[n >= split]
    slot[:len(a)] = a
    if len(b):
        slot[C - len(b):] = b[::-1]
    nA, nB = -(-len(a) // 64), -(-len(b) // 64)
    blocks = list(range(nA)) + [k for k in range(C // 64 - nB, C // 64) if k >= nA]
    return [slot[64 * k:64 * k + 64][slot[64 * k:64 * k + 64] > 0] for k in blocks]


def main():
    import pfc_pkg
    import helpers as H
    pfc = pfc_pkg.load()
    n_poses = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    C = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    w = pfc.configs.c3_blob_tool(n_poses)
    clip_n = np.concatenate([np.asarray(r.clip_n) for r in H.oracle_run(pfc, w, debug=True)])
    kept = clip_n[clip_n >= 3]
    print(f"{n_poses} poses: {len(clip_n)} candidates, {len(kept)} kept polygons, mean n {kept.mean():.2f}; "
          + ", ".join(f"n={k}: {100.0 * np.mean(kept == k):.1f} %" for k in range(3, int(kept.max()) + 1)))
    base = None
    for split in (0, 4, 5, 6):
        n_piece = iters = lanes = 0
        for c0 in range(0, len(clip_n), C):
            n = clip_n[c0:c0 + C]
            for p in pieces(n[n >= 3], C, split):
                n_piece += 1
                iters += int(p.max())
                lanes += len(p)
        if base is None:
            base = (n_piece, iters)
        print(f"bin_split {split}: {n_piece} pieces of {lanes / n_piece:.1f} polygons, {iters / n_piece:.2f} fan iterations per piece; "
              f"fan iterations and vertex slots read {100.0 * (iters / base[1] - 1.0):+.1f} %, pieces {100.0 * (n_piece / base[0] - 1.0):+.1f} % against the dense fill")


if __name__ == "__main__":
    main()
