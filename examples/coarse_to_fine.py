#!/usr/bin/env python3
"""Coarse-to-fine continuation inside one mixed-shape batch: the ground state of a harmonic well is solved on a 32^3 grid, its
wavefunction is resampled ON THE DEVICE onto the 64^3 member next to it (Batch.resample_phi(("member", 0), ...): no download, no
host copy, no upload), and the fine member is solved from there -- beside a 64^3 member that starts from the Boolean condition, to
show what the continuation saves.  Both grids cover the same box (dn halves as N doubles).

    python examples/coarse_to_fine.py [--coarse 32] [--fine 64]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import wafer_amd


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--coarse", type=int, default=32)
    ap.add_argument("--fine", type=int, default=64)
    ap.add_argument("--tolerance", type=float, default=1e-9)
    a = ap.parse_args()
    box = 12.0
    def par(n):
        dn = box / n
        return wafer_amd.Params(n, n, n, dn=dn, dt=dn * dn / 4.0, mass=1.0)
    members = [par(a.coarse), par(a.fine), par(a.fine)]   # 0: coarse, 1: fine, continued, 2: fine, from scratch
    with wafer_amd.Batch(members, mixed_shapes=True) as b:
        for m in range(3):
            b.set_potential(m, "Harmonic")
            b.set_initial_condition(m, "Boolean")
        # the coarse member alone: evolve block by block until its energy settles (the others are not in the mask)
        steps = {0: 0, 1: 0, 2: 0}

        def settle(mask, block=50):
            last = [None] * 3
            while True:
                obs = b.observables()
                b.normalise([o["norm2"] for o in obs], active=mask)
                e = [o["energy"] / o["norm2"] for o in obs]
                going = [m for m in range(3) if mask[m] and (last[m] is None or abs(e[m] - last[m]) >= a.tolerance)]
                if not going:
                    return e
                last = [e[m] if mask[m] else last[m] for m in range(3)]
                run = [1 if m in going else 0 for m in range(3)]
                mask = run
                b.evolve(block, active=run)
                for m in going:
                    steps[m] += block

        e = settle([1, 0, 0])
        print(f"coarse {a.coarse}^3: E = {e[0]:.9f} after {steps[0]} steps")
        b.resample_phi(("member", 0), active=[0, 1, 0])      # coarse -> fine, on the device, one launch
        e = settle([0, 1, 1])
        print(f"fine {a.fine}^3 continued from the coarse state: E = {e[1]:.9f} after {steps[1]} steps")
        print(f"fine {a.fine}^3 from the Boolean start:          E = {e[2]:.9f} after {steps[2]} steps")


if __name__ == "__main__":
    main()
