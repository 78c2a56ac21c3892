"""Kernel time of the search's producer kernels (k_pack, k_pack_twin, k_pack_dual, k_prep_epi6) per launch shape and per family,
from a `tools/kstats_grid.py <db> 400` listing of a `bench.py --profile --full --steps 3 --warmup 2` trace (6 calibrations).
With the counter csv files of a FETCH_SIZE and a WRITE_SIZE pass (`rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format
csv`, one pass each) it adds the memory-side bytes per launch -- FETCH_SIZE x 2 (gfx950 counts half of a wide streaming read,
MI355X_MICROARCH.md) + WRITE_SIZE, both in KB -- and the rate they make over the traced time.

With the stderr of a `bench.py --profile --steps 1 --warmup 1 --no-roofline --tune 4=2` run (`--attrib`: launch_pack prints stage,
shape, layout and grid of every k_pack / k_pack1 launch) it labels the k_pack rows with stage and class: a row is matched to
the printed launches whose work-items, times a member count of a grouped launch, give the row's grid.

    python tools/producer_table.py <kstats_grid listing> [calibrations] [--fetch F.csv --write W.csv] [--attrib stderr.txt]
"""
import argparse
import csv
import re

FAMILIES = ("k_pack_twin", "k_pack_dual", "k_prep_epi6", "k_pack")     # (k_pack last: the others start with it)
LINE = re.compile(r"^\s+(\S.*?\))\s+\((\d+), (\d+), (\d+), \d+, \d+, \d+\)\s+n=\s*(\d+) avg=\s*([\d.]+) us")


def family(name):
    name = name.replace("void ", "").replace("p4v::", "")
    return next((f for f in FAMILIES if name.startswith(f)), None)


def entry(name):
    """Entry point of a kernel name without its template arguments: k_pack_g, k_pack1_g, k_pack1, ..."""
    return name.replace("void ", "").replace("p4v::", "").split("(")[0].split("<")[0]


def counter_means(path, counter):
    """Mean counter value (KB) per (family, entry point, total work-items)."""
    acc = {}
    if not path:
        return acc
    with open(path) as fh:
        for r in csv.DictReader(fh):
            fam = family(r["Kernel_Name"])
            if fam is None or r["Counter_Name"] != counter:
                continue
            key = (fam, entry(r["Kernel_Name"]), int(r["Grid_Size"]))
            s, n = acc.get(key, (0.0, 0))
            acc[key] = (s + float(r["Counter_Value"]), n + 1)
    return {k: s / n for k, (s, n) in acc.items()}


PRINT = re.compile(r"\[p4v\] (k_pack1?) stage (\d+): Z (\d+) Rp (\d+) Kp (\d+) C (\d+) crange (\d) done (\d)(?: live_max (-?\d+))? layout (\d) "
                   r"(?:blocks (\d+)|grid (\d+) x (\d+))")
MAX_MEMBERS = 16        # GroupArgs<PackParams>::CAP is 15: a grouped launch holds at most that many members
STAGES = {0: "-", 1: "A", 2: "B1", 3: "B2", 4: "A2"}


def attribution(path):
    """{work-items of one member's launch: {label}} from the launch_pack prints; label = stage / class / layout / C."""
    out = {}
    if not path:
        return out
    for line in open(path):
        m = PRINT.search(line)
        if not m:
            continue
        kern, stage, C, crange, live, layout = m.group(1), int(m.group(2)), int(m.group(6)), m.group(7) == "1", m.group(9), m.group(10)
        if m.group(11):
            blocks, groups = int(m.group(11)), -(-C // 10)
        else:
            blocks, groups = int(m.group(12)), int(m.group(13))
        cls = "pruned" if crange else "single" if C == 1 else "unpruned"
        if crange and live not in (None, "-1"):
            cls += f"(known {live})"
        label = f"{STAGES.get(stage, stage)} {cls} L{layout} C{C}"
        out.setdefault((kern, -(-blocks * groups // 8) * 8 * 256, blocks * groups * 256), set()).add(label)
    return out


def labels(attr, name, grid):
    """Labels of the printed launches that make a launch of `grid` work-items: one launch, or 2..MAX_MEMBERS grouped members of one shape."""
    kern = "k_pack1" if name.startswith("k_pack1") else "k_pack"
    grouped = "_g" in name.split("(")[0]
    found = set()
    for (k, padded, plain), lab in attr.items():
        if k != kern:
            continue
        if grouped and grid % padded == 0 and 2 <= grid // padded <= MAX_MEMBERS:
            found |= {f"{l} x{grid // padded}" for l in lab}
        if not grouped and grid == plain:
            found |= lab
    return " | ".join(sorted(found)) if found else "?"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("calibs", nargs="?", type=int, default=6)
    ap.add_argument("--fetch", default="")
    ap.add_argument("--write", default="")
    ap.add_argument("--attrib", default="")
    a = ap.parse_args()
    fetch, write = counter_means(a.fetch, "FETCH_SIZE"), counter_means(a.write, "WRITE_SIZE")
    attr = attribution(a.attrib)
    rows = []
    for line in open(a.listing):
        m = LINE.match(line)
        if not m or family(m.group(1)) is None:
            continue
        name = m.group(1)
        n, avg = int(m.group(5)), float(m.group(6))
        rows.append((family(name), name, int(m.group(2)), int(m.group(3)), n, avg, n * avg / 1e3 / a.calibs))
    rows.sort(key=lambda r: -r[-1])
    print(f"producer kernels, {a.calibs} calibrations per trace; grid = total work-items (x, y) of the launch")
    bytes_cols = bool(fetch or write)
    hdr = f"{'family':12s} {'kernel':44s} {'grid_x':>10s} {'y':>3s} {'n':>4s} {'avg us':>8s} {'ms/calib':>9s}"
    print(hdr + (f" {'read MB':>9s} {'write MB':>9s} {'TB/s':>6s}" if bytes_cols else "") + ("  stage class layout C x members" if attr else ""))
    for fam, name, gx, gy, n, avg, per in rows:
        line = f"{fam:12s} {name:44s} {gx:10d} {gy:3d} {n:4d} {avg:8.1f} {per:9.3f}"
        if bytes_cols:
            key = (fam, entry(name), gx * gy)
            if key in fetch or key in write:
                rd, wr = fetch.get(key, 0.0) * 2048.0, write.get(key, 0.0) * 1024.0
                line += f" {rd / 1e6:9.1f} {wr / 1e6:9.1f} {(rd + wr) / (avg * 1e-6) / 1e12:6.2f}"
            else:
                line += f" {'-':>9s} {'-':>9s} {'-':>6s}"
        if attr and fam == "k_pack":
            line += "  " + labels(attr, name.replace("void ", "").replace("p4v::", ""), gx * gy)
        print(line)
    print()
    total = 0.0
    for fam in FAMILIES:
        t = sum(r[-1] for r in rows if r[0] == fam)
        launches = sum(r[4] for r in rows if r[0] == fam) / a.calibs
        total += t
        print(f"{fam:12s} {t:7.2f} ms per calibration, {launches:6.1f} launches")
    print(f"{'all four':12s} {total:7.2f} ms per calibration")


if __name__ == "__main__":
    main()
