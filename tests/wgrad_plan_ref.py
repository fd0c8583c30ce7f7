"""pbn_spconv_wgrad's launch plan restated in Python, independently of csrc/wgrad_plan.h: the statement that
tests/golden/wgrad_plans.json was recorded from (make_wgrad_plan_golden.py), that tests/test_wgrad_plan_cpu.py holds
pbn_spconv_wgrad_plan to, and that tests/test_grad_parity_gpu.py compares with the library's answer before every exact case."""
import os

import torch


def cdiv(a, b):
    return -(-a // b)


def wgrad_plan(dtype, ld_x, ld_g, x_ptr, g_ptr, cin, cout, n_pairs, K, ident, ws_bytes):
    """pbn_spconv_wgrad's dispatch restated (csrc/wgrad_plan.h): (form, WA, WB, small_level, splits).  Reads the same
    environment knobs; PBN_WGRAD_FORM as this process saw it at start."""
    env = lambda k: int(os.environ[k]) if os.environ.get(k) else 0
    form_env = env("PBN_WGRAD_FORM")
    form16 = (form_env != 32 and dtype != torch.float32 and ld_x % 8 == 0 and ld_g % 8 == 0 and ld_x >= (cin + 7) // 8 * 8
              and ld_g >= (cout + 7) // 8 * 8 and ((x_ptr | g_ptr) & 15) == 0)
    ring = form16
    wa = wb = 0
    small = False
    if form16:
        cit, cot = cdiv(cin, 16), cdiv(cout, 16)
        wa = 4 if cit >= 7 else (cit + 1) // 2
        wb = 4 if cot >= 7 else (cot + 1) // 2
        small = ring and n_pairs // K < 3000 and cdiv(cit, 2 * wa) * cdiv(cot, 2 * wb) * K < 256
        maxt = env("PBN_WGRAD_MAXT") or (2 if small else 4)
        wa, wb = min(wa, maxt), min(wb, maxt)
        strips = cdiv(cit, 2 * wa) * cdiv(cot, 2 * wb)
    else:
        strips = cdiv(cin, 16) * cdiv(cout, 64)
    want, minp = env("PBN_WGRAD_WGS"), env("PBN_WGRAD_MIN_PAIRS")
    target = want if want > 0 else (1024 if ring else 2048)
    min_pairs = minp if minp > 0 else (256 if ring else 512)
    ppo = n_pairs // K + 1
    splits = target // (strips * K) + 1
    splits = min(splits, ppo // min_pairs + 1)
    n_out = K * cin * cout
    if ring:
        splits = min(splits, (32 << 20) // (4 * n_out) + 1)
    if small and want <= 0:
        splits = 1
    splits = min(splits, ws_bytes // (4 * n_out), 64)
    splits = max(splits, 1)
    form = ("ring%d%d%s" % (wa, wb, "i" if ident else "")) if ring else "w32"
    return form, wa, wb, small, splits
