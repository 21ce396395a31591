"""Tables of profiles/norm_f64/README.md from the JSON that tests/test_gpu_norm_f64.py writes:

    TBAMD_NORM_F64_REPORT=report.json python -m pytest tests/test_gpu_norm_f64.py -m gpu
    python profiles/norm_f64/summarize.py report.json
"""
import json
import sys
from collections import defaultdict


def fam(case):
    c = case[0]
    return "GN/IN" if c.startswith("gn") else "BN"


def main(path):
    recs = json.load(open(path))
    blocks, vecs, kinks, over, cond = defaultdict(list), defaultdict(list), [], [], []
    for r in recs:
        case, out = r["case"], r["out"]
        tag = case[0]
        if out == "kink_share":
            kinks.append(r)
        elif out == "var_outlier_row0":
            cond.append(r)
        elif "E_el" in r:
            if tag in ("offset", "gn-offset"):
                cond.append(r)
            vecs[(fam(case), out, r["dtype"])].append(r)
            if r["used_el"] > 1.0:
                over.append(r)
        else:
            if tag in ("offset", "gn-offset"):
                cond.append(r)
            else:
                blocks[(fam(case), out, r["dtype"])].append(r)
    print("## y / dx / dres (largest block error per output and dtype; well-centred inputs)\n")
    print("| op | output | dtype | cases | max E | max E_stock | largest E / bound | same, paired per block |")
    print("|---|---|---|---|---|---|---|---|")
    for k in sorted(blocks):
        v = blocks[k]
        es = [r["E_stock"] for r in v if r["E_stock"] is not None]
        pr = [r["used_paired"] for r in v if r.get("used_paired") is not None]
        print("| %s | %s | %s | %d | %.2e | %s | %.2f | %s |" % (
            k[0], k[1], k[2], len(v), max(r["E"] for r in v), "%.2e" % max(es) if es else "-",
            max(r["used"] for r in v), "%.2f" % max(pr) if pr else "-"))
    print("\n## per-channel vectors (relative L2 over the vector | elementwise relative maximum)\n")
    print("| op | output | dtype | checks | max E (L2) | its E_stock | max E/E_stock (L2) | max E (elementwise) "
          "| max E/E_stock (elementwise) | largest E / bound (L2) | (elementwise, margin 4) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for k in sorted(vecs):
        v = vecs[k]
        w = max(v, key=lambda r: r["E"])
        print("| %s | %s | %s | %d | %.2e | %.2e | %.2f | %.2e | %.2f | %.2f | %.2f |" % (
            k[0], k[1], k[2], len(v), w["E"], w["E_stock"], max((r["ratio"] or 0) for r in v),
            max(r["E_el"] for r in v), max((r["ratio_el"] or 0) for r in v), max(r["used"] for r in v),
            max(r["used_el"] for r in v)))
    print("\n## conditioning cases\n")
    print("| case | output | E | E_stock | kappa (max) | E / bound |")
    print("|---|---|---|---|---|---|")
    for r in cond:
        print("| %s | %s | %.3e | %s | %s | %.3f |" % (
            " ".join(map(str, r["case"])), r["out"], r["E"],
            "%.3e" % r["E_stock"] if r.get("E_stock") is not None else "-",
            "%.0f" % r["kappa"] if "kappa" in r else "-", r["used"]))
    print("\n## kink-excluded elements\n")
    nz = [r for r in kinks if r["n"]]
    print("%d ReLU / leaky-ReLU cases; %d exclude anything; largest share %.2e (%s: %d of %d)." % (
        len(kinks), len(nz), *(lambda r: (r["E"], " ".join(map(str, r["case"])), r["n"], r["numel"]))(
            max(kinks, key=lambda r: r["E"]))))
    for r in nz:
        print("- %s: %d of %d (%.2e)" % (" ".join(map(str, r["case"])), r["n"], r["numel"], r["E"]))
    print("\n## elementwise margins above 4 (EL_MARGIN = twice the measured share of margin 4, times 4)\n")
    for r in sorted(over, key=lambda r: (r["case"], r["out"])):
        print("    (%r, %r): %.1f,  # E=%.2e E_stock=%.2e" % (
            tuple(r["case"]), r["out"], 8.0 * r["used_el"] * 1.0001 + 0.05, r["E_el"], r["E_el_stock"]))


if __name__ == "__main__":
    main(sys.argv[1])
