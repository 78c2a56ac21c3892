"""Golden fixtures of the Linear classes with the cosine metric and weight column blocks / activation blocks (n_H, n_a > 1):
tests/golden/linblk_*.npz.

A CPU tool: it runs the REFERENCE implementation (oracle.gen_golden._install_shims puts its checkout on the path) through the
existing generators gen_linear / gen_ptqsl_linear, which hand n_V / n_H / n_a through to the reference's constructors, and
records every score table the reference fed to argmax, the final intervals and the quantised output.

    python tools/gen_golden_linblk.py [--out DIR] [name ...]

The widths are low on purpose: a cosine score is S - defect (S = images for the batching class, 1 for the non-batching one),
and on 8-bit data the defect is O(1e-5) -- no tolerance tells a wrong block scale from a right one there.

What the cases cover (shape_x = batch, tokens, in_features):
  linblk_cos_v2h2a3_w4a4                K = 24 cut at 8 / 12 / 16: four segments; bias; 2 rounds
  linblk_cos_v3h2a5_m140_k140_oc150     six segments; 140 samples cross a 128-column tile; V blocks of 50 rows in a 64-row slab
  linblk_cos_v1h2a1_k140_w6_nobias      segments of 70 = two k-tiles each; no bias; 6 bit
  linblk_cos_v3h1a2_w8a4                activation blocks only; mixed widths
  linblk_ptqsl_cos_v2h2a2               non-batching class: one mean over batch and tokens
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COS = dict(metric="cosine", eq_alpha=0.5, eq_beta=1.2, eq_n=100, search_round=2)

# (generator, name, arguments)
CASES = [
    ("gen_linear", "linblk_cos_v2h2a3_w4a4",
     dict(shape_x=(3, 11, 24), oc=16, n_V=2, n_H=2, n_a=3, w_bit=4, a_bit=4, seed=200, **COS)),
    ("gen_linear", "linblk_cos_v3h2a5_m140_k140_oc150",
     dict(shape_x=(2, 70, 140), oc=150, n_V=3, n_H=2, n_a=5, w_bit=4, a_bit=4, seed=201, store_qf=False,
          **dict(COS, search_round=1))),
    ("gen_linear", "linblk_cos_v1h2a1_k140_w6_nobias",
     dict(shape_x=(2, 19, 140), oc=40, n_V=1, n_H=2, n_a=1, w_bit=6, a_bit=6, seed=202, bias=False, **COS)),
    ("gen_linear", "linblk_cos_v3h1a2_w8a4",
     dict(shape_x=(3, 17, 96), oc=48, n_V=3, n_H=1, n_a=2, w_bit=8, a_bit=4, seed=204, **COS)),
    ("gen_ptqsl_linear", "linblk_ptqsl_cos_v2h2a2",
     dict(shape_x=(3, 11, 24), oc=16, n_V=2, n_H=2, n_a=2, w_bit=4, a_bit=4, seed=203, **COS)),
]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="output directory (default: tests/golden)")
    ap.add_argument("names", nargs="*", help="fixtures to (re)generate (default: all)")
    args = ap.parse_args(argv)
    import oracle.gen_golden as gg
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        gg.OUT = args.out
    gg._install_shims()
    for gen, name, kw in CASES:
        if args.names and name not in args.names:
            continue
        getattr(gg, gen)(name, **kw)
        print(f"[gen] {name}: {os.path.getsize(os.path.join(gg.OUT, name + '.npz'))} bytes", flush=True)


if __name__ == "__main__":
    main()
