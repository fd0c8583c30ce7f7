"""Generates tests/golden/conv_family.json: what pbn_spconv_family answers (0 workgroup-tile, 1 wave-autonomous, 2 row-stationary)
over a small table of launch shapes, default environment.

Recorded at the commit BEFORE the automatic family choice of csrc/spconv.hip became one ordered table that both the launch and
pbn_spconv_family read; tests/test_conv_family.py asks the library again and compares, so whoever reorders or rewrites that
table has to reproduce every answer.  The function is host code: no GPU is needed, only the built library.

The table: dtypes f32 and bf16, with and without a map, K in {1, 8, 27, 125}, the (vecs per offset, padded output channels)
pairs of the recorded MinkUNet plans of that dtype (unet_plans.json), and row counts around every threshold of the choice
(64 / 65: tile height; 20 000 / 30 000: row-stationary from, wave-autonomous up to; 146 038: the bench scene).

Run from the repo root:  python tests/golden/make_conv_family_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "conv_family.json")
DTYPES = {"f32": 0, "bf16": 1}                      # pbn_dtype
KS = (1, 8, 27, 125)
N_OUT = (0, 1, 64, 65, 4000, 19999, 20000, 29999, 30000, 146038)


def channel_pairs(dtype_name):
    """Sorted distinct (vpo, cout_p) of every op of the recorded inference plans of this dtype."""
    with open(os.path.join(HERE, "unet_plans.json")) as f:
        plans = json.load(f)["inference"]
    pairs = set()
    for name, p in plans.items():
        if "-%s-" % dtype_name in name:
            iv, ic = p["op_fields"].index("vpo"), p["op_fields"].index("cout_p")
            pairs.update((op[iv], op[ic]) for op in p["ops"])
    return sorted(pairs)


def cases():
    """[dtype name, has_map, K, vpo, cout_p, n_out] in a fixed order."""
    return [[dn, has_map, k, vpo, cout_p, n]
            for dn in sorted(DTYPES) for has_map in (0, 1) for k in KS for vpo, cout_p in channel_pairs(dn) for n in N_OUT]


def ask(lib, case):
    dn, has_map, k, vpo, cout_p, n = case
    return int(lib.pbn_spconv_family(n, k, vpo, (k * vpo + 3) // 4, cout_p, DTYPES[dn], has_map))


def main():
    from pbnet_amd import _native
    lib = _native.lib()
    rows = cases()
    fam = [ask(lib, c) for c in rows]
    with open(OUT, "w") as f:
        json.dump({"fields": ["dtype", "has_map", "K", "vpo", "cout_p", "n_out"], "cases": rows, "family": fam}, f,
                  separators=(",", ":"))
        f.write("\n")
    print(len(rows), "cases;", {v: fam.count(v) for v in sorted(set(fam))})


if __name__ == "__main__":
    main()
