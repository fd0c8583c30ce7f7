"""CPU tier: the host-only paths of the device AP table (pbn_ap_table_*): the workspace query runs without a device and grows
with both capacities, and every argument check returns before any launch -- the pointers below are fake and never dereferenced,
as in tests/test_abi.py."""
import numpy as np

from pbnet_amd import _native as N
from pbnet_amd import evaluate as E

FAKE = 1 << 20                                        # 256-byte aligned, never touched


def tables(n_classes=18, n_overlaps=10):
    classes, overlaps = N.ApClassIds(), N.ApOverlaps()
    classes.n, overlaps.n = n_classes, n_overlaps
    for i, c in enumerate(E.VALID_CLASS_IDS):
        classes.id[i] = int(c)
    for i, th in enumerate(E.OVERLAPS):
        overlaps.th[i] = float(th)
    return classes, overlaps


def test_workspace_query_is_host_only_and_grows_with_both_capacities():
    lib = N.lib()
    small = lib.pbn_ap_table_workspace_bytes(16, 1024)
    assert 0 < small < lib.pbn_ap_table_workspace_bytes(4096, 1024) and small < lib.pbn_ap_table_workspace_bytes(16, 1 << 20)
    assert lib.pbn_ap_table_workspace_bytes(0, 1024) == 0 and lib.pbn_ap_table_workspace_bytes(16, 0) == 0
    assert lib.pbn_ap_table_workspace_bytes(16, 1 << 30) == 0
    assert lib.pbn_ap_table_lds_entries() >= 256


def test_struct_sizes_are_the_headers():
    import ctypes
    assert ctypes.sizeof(N.ApClassIds) == 4 * (1 + N.AP_MAX_CLASSES) and ctypes.sizeof(N.ApOverlaps) == 8 + 8 * N.AP_MAX_OVERLAPS
    assert len(E.CLASS_LABELS) <= N.AP_MAX_CLASSES and len(E.OVERLAPS) <= N.AP_MAX_OVERLAPS


def test_argument_checks_return_before_any_launch():
    lib, vp = N.lib(), N.c_vp
    need = lib.pbn_ap_table_workspace_bytes(16, 1024)
    classes, overlaps = tables()

    def add(ws=FAKE, nbytes=need, rec_cap=16, entry_cap=1024, state=FAKE, log=FAKE, log_words=100, tag_base=0, classes=classes,
            overlaps=overlaps, min_region=100):
        return lib.pbn_ap_table_add_log(vp(ws), nbytes, rec_cap, entry_cap, vp(state), vp(log), log_words, tag_base, classes,
                                        overlaps, min_region, None)

    assert add(ws=0) == N.PBN_ERR_ARG and add(state=0) == N.PBN_ERR_ARG and add(log=0) == N.PBN_ERR_ARG
    assert add(rec_cap=0) == N.PBN_ERR_ARG and add(entry_cap=0) == N.PBN_ERR_ARG and add(log_words=-1) == N.PBN_ERR_ARG
    assert add(tag_base=-1) == N.PBN_ERR_ARG and add(min_region=-1) == N.PBN_ERR_ARG
    assert add(classes=tables(0)[0]) == N.PBN_ERR_ARG and add(classes=tables(33)[0]) == N.PBN_ERR_ARG
    assert add(overlaps=tables(18, 0)[1]) == N.PBN_ERR_ARG and add(overlaps=tables(18, 17)[1]) == N.PBN_ERR_ARG
    bad = tables()[1]
    bad.th[3] = float("nan")
    assert add(overlaps=bad) == N.PBN_ERR_ARG
    bad = tables()[0]
    bad.id[2] = -5
    assert add(classes=bad) == N.PBN_ERR_ARG
    bad.id[2] = 0                                       # id 0 is the unannotated id: always a void column, never a class
    assert add(classes=bad) == N.PBN_ERR_ARG
    assert add(entry_cap=1 << 30) == N.PBN_ERR_RANGE and add(log_words=1 << 31) == N.PBN_ERR_RANGE
    assert add(nbytes=need - 1) == N.PBN_ERR_WORKSPACE and add(rec_cap=17) == N.PBN_ERR_WORKSPACE

    def finish(ws=FAKE, nbytes=need, rec_cap=16, entry_cap=1024, n_classes=18, n_overlaps=10, out=FAKE):
        return lib.pbn_ap_table_finish(vp(ws), nbytes, rec_cap, entry_cap, n_classes, n_overlaps, vp(out), vp(FAKE), vp(FAKE),
                                       vp(FAKE), vp(FAKE), None)

    assert finish(ws=0) == N.PBN_ERR_ARG and finish(out=0) == N.PBN_ERR_ARG
    assert finish(n_classes=0) == N.PBN_ERR_ARG and finish(n_overlaps=17) == N.PBN_ERR_ARG and finish(rec_cap=-1) == N.PBN_ERR_ARG
    assert finish(entry_cap=1 << 30) == N.PBN_ERR_RANGE and finish(nbytes=need - 1) == N.PBN_ERR_WORKSPACE

    reset = lambda ws, nbytes, rec_cap, entry_cap: lib.pbn_ap_table_reset(vp(ws), nbytes, rec_cap, entry_cap, None)   # noqa: E731
    assert reset(0, need, 16, 1024) == N.PBN_ERR_ARG and reset(FAKE, need, 0, 1024) == N.PBN_ERR_ARG
    assert reset(FAKE, need - 1, 16, 1024) == N.PBN_ERR_WORKSPACE and reset(FAKE, need, 16, 1 << 30) == N.PBN_ERR_RANGE


def test_config_default_is_off():
    from pbnet_amd.config import get_config
    assert get_config().device_ap_table is False and np.isclose(E.OVERLAPS[2], 0.6) and E.OVERLAPS[2] != 0.6
