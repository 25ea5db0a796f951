"""Host wall-clock cost of the host-pointer forms that stage through the context's block (pfc_items_from_bodies,
pfc_dual_seeds_from_bodies, pfc_local_jacobian, pfc_apply_local_jacobian, pfc_scatter_generalized[_dual], pfc_contact_surface[_fric])
on the small scene of tests/helpers.py (HostFormsCase): uploads, launch, downloads and the synchronisation, as a C caller sees them
plus the ctypes call.  Medians over `reps` blocks of 20 calls after a warm-up, in microseconds; one JSON line at the end.

usage: python scripts/host_forms_rate.py [reps]      PFC_LIB=<variant> measures another build of the library."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import pfc_pkg


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    pfc = pfc_pkg.load()
    import helpers as H
    case = H.HostFormsCase(pfc)
    m = case.handle(pfc)
    out = {}
    for form in H.HOST_FORMS_ORDER:
        for _ in range(5):
            case.run(pfc, m, form)
        blocks = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(20):
                case.run(pfc, m, form)
            blocks.append((time.perf_counter() - t0) / 20 * 1e6)
        out[form] = float(np.median(blocks))
        print(f"{form:>15s}: {out[form]:9.1f} us per call (min {min(blocks):9.1f}, max {max(blocks):9.1f})", flush=True)
    m.close()
    print(json.dumps({"host_forms_us": out}))


if __name__ == "__main__":
    main()
