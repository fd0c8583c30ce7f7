"""Generates tests/golden/wgrad_plans.json: the launch plan of the weight gradient (kernel form, WA, WB, small_level, strips,
pair splits) over a table of call shapes, with PBN_WGRAD_FORM unset and with PBN_WGRAD_FORM=32, every other PBN_WGRAD_* knob
unset.

Recorded from the Python statement of the dispatch (tests/wgrad_plan_ref.py) as it stood, inside tests/test_grad_parity_gpu.py,
at the commit BEFORE the plan became one host function (csrc/wgrad_plan.h) that both the launch and pbn_spconv_wgrad_plan
read; tests/test_wgrad_plan_cpu.py asks that statement and the library again and compares, so whoever rewrites either has to
reproduce every answer.  No GPU and no library are needed to record.

The table: dtypes f32 / bf16 / f16; slab bases aligned to 16 bytes or not; ld % 8 == 0 or not; cin, cout over the 1 -> 2 -> 3 ->
4 tile steps, the `cit >= 7` rule and channel tails; K in {1, 8, 27, 125}; pairs per offset around the small_level threshold
(2999 / 3000) and from none to the bench scene's stride-1 map; workspace absent / one dW slab / the full 64; pair lists, and
identity pairs where K = 1.  The full product (about 280 000 shapes) is thinned by a fixed multiplicative hash of the shape's
position in it: one in 16 of the shapes that can reach k_wgrad_ring, one in 160 of those that only reach k_wgrad<T>.

Run from the repo root:  python tests/golden/make_wgrad_plan_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

OUT = os.path.join(HERE, "wgrad_plans.json")
FIELDS = ["dtype", "aligned", "ld8", "cin", "cout", "K", "pairs_per_offset", "workspace", "identity"]
ANSWER = ["form", "wa", "wb", "small", "strips", "splits"]
DTYPES = {"f32": 0, "bf16": 1, "f16": 2}            # pbn_dtype
CHANNELS = (3, 6, 20, 32, 48, 56, 64, 90, 96, 112, 120, 128, 136, 256)
KS = (1, 8, 27, 125)
PAIRS = (0, 1, 31, 100, 2999, 3000, 12000, 150000)
WORKSPACE = (0, 1, 2)                               # absent, one dW slab, pbn_spconv_wgrad_workspace_bytes
KNOBS = ("PBN_WGRAD_MAXT", "PBN_WGRAD_WGS", "PBN_WGRAD_MIN_PAIRS", "PBN_WGRAD_DBG")
BASE = 1 << 20                                      # a 16-byte aligned address


def cases():
    """The thinned table, in a fixed order."""
    rows, i = [], 0
    for dn in ("f32", "bf16", "f16"):
        for aligned in (1, 0):
            for ld8 in (1, 0):
                keep_one_in = 16 if (dn != "f32" and aligned and ld8) else 160
                for cin in CHANNELS:
                    for cout in CHANNELS:
                        for k in KS:
                            for ident in ((0, 1) if k == 1 else (0,)):
                                for ppo in PAIRS:
                                    for ws in WORKSPACE:
                                        i += 1
                                        if ((i * 2654435761) & 0xffffffff) >> 12 < (1 << 20) // keep_one_in:
                                            rows.append([dn, aligned, ld8, cin, cout, k, ppo, ws, ident])
    return rows


def call_shape(case):
    """The arguments a case stands for.  A misaligned base / an ld % 8 != 0 sits on the x slab for K = 1 / 27, on g otherwise."""
    dn, aligned, ld8, cin, cout, k, ppo, ws, ident = case
    on_x = k in (1, 27)
    ld_x = (cin + 7) // 8 * 8 + (0 if ld8 or not on_x else 4)
    ld_g = (cout + 7) // 8 * 8 + (0 if ld8 or on_x else 2)
    x_ptr = BASE + (0 if aligned or not on_x else 2)
    g_ptr = BASE + (0 if aligned or on_x else 2)
    n_out = k * cin * cout
    return dict(dtype=dn, ld_x=ld_x, ld_g=ld_g, x_ptr=x_ptr, g_ptr=g_ptr, cin=cin, cout=cout, n_pairs=ppo * k, K=k, ident=ident,
                has_ws=int(ws > 0), ws_bytes=4 * n_out * (0, 1, 64)[ws])


def strips_of(case, wa, wb):
    """Tile strips of one offset (the reference statement does not return them): its own formula, from its WA / WB."""
    cin, cout = case[3], case[4]
    cdiv = lambda a, b: -(-a // b)
    if wa:
        return cdiv(cdiv(cin, 16), 2 * wa) * cdiv(cdiv(cout, 16), 2 * wb)
    return cdiv(cin, 16) * cdiv(cout, 64)


def reference_plans(rows, form_env, plan_fn=None):
    """[form, wa, wb, small, strips, splits] per case from the Python statement, under PBN_WGRAD_FORM = form_env (None: unset)."""
    import torch
    if plan_fn is None:
        import wgrad_plan_ref
        plan_fn = wgrad_plan_ref.wgrad_plan
    tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
    set_knobs = [k for k in KNOBS if os.environ.get(k)]
    if set_knobs:
        raise RuntimeError("the record holds with these unset: " + ", ".join(set_knobs))
    saved = os.environ.pop("PBN_WGRAD_FORM", None)
    try:
        if form_env is not None:
            os.environ["PBN_WGRAD_FORM"] = form_env
        out = []
        for c in rows:
            s = call_shape(c)
            form, wa, wb, small, splits = plan_fn(tdt[s["dtype"]], s["ld_x"], s["ld_g"], s["x_ptr"], s["g_ptr"], s["cin"], s["cout"],
                                                  s["n_pairs"], s["K"], bool(s["ident"]), s["ws_bytes"] if s["has_ws"] else 0)
            out.append([form, wa, wb, int(small), strips_of(c, wa, wb), splits])
        return out
    finally:
        os.environ.pop("PBN_WGRAD_FORM", None)
        if saved is not None:
            os.environ["PBN_WGRAD_FORM"] = saved


def ask(lib, plan_struct, case):
    """(rc, [form, wa, wb, small, strips, splits], grid) from pbn_spconv_wgrad_plan; an absent workspace keeps its byte count, which
    the library must ignore."""
    import ctypes
    s = call_shape(case)
    p = plan_struct()
    full = 4 * s["K"] * s["cin"] * s["cout"] * 64
    rc = lib.pbn_spconv_wgrad_plan(DTYPES[s["dtype"]], s["ld_x"], s["ld_g"], int(((s["x_ptr"] | s["g_ptr"]) & 15) == 0), s["ident"],
                                   s["K"], s["n_pairs"], s["cin"], s["cout"], s["has_ws"], s["ws_bytes"] if s["has_ws"] else full,
                                   ctypes.byref(p))
    form = ("ring%d%d%s" % (p.wa, p.wb, "i" if s["ident"] else "")) if p.form == 1 else "w32"
    return rc, [form, p.wa, p.wb, p.small_level, p.strips, p.splits], p.grid


def main():
    rows = cases()
    plans = {"default": reference_plans(rows, None), "form32": reference_plans(rows, "32")}
    with open(OUT, "w") as f:
        json.dump({"fields": FIELDS, "answer": ANSWER, "cases": rows, "plans": plans}, f, separators=(",", ":"))
        f.write("\n")
    forms = sorted(set(p[0] for p in plans["default"]))
    print(len(rows), "cases;", len(forms), "forms;", sum(p[3] for p in plans["default"]), "small_level;",
          sum(p[5] > 1 for p in plans["default"]), "split")


if __name__ == "__main__":
    main()
