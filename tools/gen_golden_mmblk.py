"""Golden fixtures of the MatMul classes with row / column sub-blocks (n_V, n_H > 1): tests/golden/mmblk_*.npz.

A CPU tool: it runs the REFERENCE implementation (oracle.gen_golden._install_shims puts its checkout on the path) through the
existing generators gen_matmul / gen_ptqsl_matmul, which hand n_V_* / n_H_* through to the reference's constructors, and
records every score table the reference fed to argmax, the final intervals and the quantised output.

    python tools/gen_golden_mmblk.py [--out DIR] [name ...]

What the cases cover (b, H, d1, d2, d3 = batch, heads, M, K, N):
  mmblk_qk_hessian_vA2hA2_vB2hB3                 ragged rows 7/6 and columns 5/5/3, coinciding K cuts
  mmblk_sv_hessian_w6_vA3hA2_vB3hB2              6 bit; K cuts at 4, 6, 8: four segments
  mmblk_sos_hessian_vB2hB2                       split-of-softmax twin on A with row blocks on B
  mmblk_qk_l2_k70_hA2_vB3                        K = 70: more than one 64-byte k-tile, cuts 24 / 35 / 48
  mmblk_empty_block                              M = 5 in 4 row blocks: a block of padding only (interval 0, no NaN)
  mmblk_sv_hessian_m133_k133_vA2hA2_vB2hB2       rows cross a 128 tile, segments of 67 / 66 = two k-tiles each (1 round)
  mmblk_ptqsl_qk_hessian_g2of3_vA2hA2_vB2hB2     non-batching class, 2 groups of 3 heads (a padding head) + sub-blocks
  mmblk_ptqsl_sos_l2_g1_vB2hB2                   non-batching split-of-softmax class, one group
and, with `mixbit` (or their names) on the command line, the mixed-width cases of oracle.gen_golden.MIXBIT_MMBLK_CASES:
  mixbit_mmblk_qk_a8b4_vA2hA2_vB2hB2             A 8 bit, B 4 bit, 2 x 2 blocks on both operands
  mixbit_mmblk_sos_a4b8_vB2hB2                   split-of-softmax A on 4 bits, B on 8 bits in 2 x 2 blocks
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_SEARCH = dict(eq_alpha=0.01, eq_beta=1.2, eq_n=100)
HESSIAN = dict(metric="hessian", search_round=2, **_SEARCH)
L2 = dict(metric="L2_norm", search_round=2, **_SEARCH)
W8 = dict(A_bit=8, B_bit=8)

# (generator, name, arguments)
CASES = [
    ("gen_matmul", "mmblk_qk_hessian_vA2hA2_vB2hB3",
     dict(b=4, H=3, d1=13, d2=8, d3=13, seed=70, n_V_A=2, n_H_A=2, n_V_B=2, n_H_B=3, **W8, **HESSIAN)),
    ("gen_matmul", "mmblk_sv_hessian_w6_vA3hA2_vB3hB2",
     dict(b=3, H=2, d1=11, d2=11, d3=8, A_bit=6, B_bit=6, seed=71, n_V_A=3, n_H_A=2, n_V_B=3, n_H_B=2, **HESSIAN)),
    ("gen_matmul", "mmblk_sos_hessian_vB2hB2",
     dict(b=4, H=3, d1=13, d2=13, d3=8, sos=True, seed=72, n_V_B=2, n_H_B=2, **W8, **HESSIAN)),
    ("gen_matmul", "mmblk_qk_l2_k70_hA2_vB3",
     dict(b=2, H=2, d1=37, d2=70, d3=21, seed=73, n_V_A=1, n_H_A=2, n_V_B=3, n_H_B=1, **W8, **L2)),
    ("gen_matmul", "mmblk_empty_block",
     dict(b=2, H=2, d1=5, d2=8, d3=5, seed=76, n_V_A=4, n_H_A=1, n_V_B=1, n_H_B=4, **W8, **HESSIAN)),
    ("gen_matmul", "mmblk_sv_hessian_m133_k133_vA2hA2_vB2hB2",
     dict(b=2, H=2, d1=133, d2=133, d3=40, seed=77, n_V_A=2, n_H_A=2, n_V_B=2, n_H_B=2, **W8,
          **dict(HESSIAN, search_round=1))),
    ("gen_ptqsl_matmul", "mmblk_ptqsl_qk_hessian_g2of3_vA2hA2_vB2hB2",
     dict(b=4, H=3, d1=13, d2=8, d3=13, seed=74, n_G_A=2, n_G_B=2, n_V_A=2, n_H_A=2, n_V_B=2, n_H_B=2, **W8, **HESSIAN)),
    ("gen_ptqsl_matmul", "mmblk_ptqsl_sos_l2_g1_vB2hB2",
     dict(b=4, H=3, d1=13, d2=13, d3=8, sos=True, seed=75, n_G_B=1, n_V_B=2, n_H_B=2, **W8, **L2)),
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
    # the mixed-width sub-block cases (prefix mixbit_: tests/test_oracle_mixbit.py, tests/test_hip_mixbit.py), on request only
    mix = [c for c in gg.MIXBIT_MMBLK_CASES if "mixbit" in args.names or c[1] in args.names]
    if mix:
        os.chdir(gg.REF)
        gg.gen_mixed_bits(mix)


if __name__ == "__main__":
    main()
