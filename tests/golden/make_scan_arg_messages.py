"""Records tests/golden/scan_arg_messages.json: what every call of tests/scan_arg_cases.py raises, as (exception class name,
message).  It was run once, at the commit before pbnet_amd/mesh.py was split into mesh.py, cloud.py and ply.py:

    python tests/golden/make_scan_arg_messages.py

No device and no library are needed.  For every case but the "device" ones the device check and the library are replaced
by stand-ins, so that a CPU tensor is not a second fault and the one fault of the case is what speaks, wherever in the
function its check stands.  The status cases drive each stage's own decode of the status word: the stand-in for the launch
writes the status value into the stage's status tensor, which lives on the CPU here.  The script looks every function up
through pbnet_amd.mesh and patches the module the function lives in, so it can be run again on a later tree; the file it
writes must not change."""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import scan_arg_cases as S  # noqa: E402
from pbnet_amd import _native as N, mesh  # noqa: E402

# where each staged entry takes its status pointer
STATUS_ARG = {"cloud_knn": 6, "thin_points": 9, "cloud_orient": 8, "cloud_upright": 16, "cloud_vote_labels": 10,
              "cloud_radius_count": 6}


class StandInLibrary:
    """Sizes only; with `status` also the one entry that is not called through _staged_call."""

    def __init__(self, status=None):
        self.status = status

    def __getattr__(self, name):
        if name == "pbn_cloud_max_k":
            return lambda: 32
        if name == "pbn_cloud_upright_max_hyp":
            return lambda: 4096
        if name.endswith("_workspace_bytes"):
            return lambda *a: 256
        if name == "pbn_cloud_radius_raw_index" and self.status is not None:
            return lambda *a: _poke(a[8], self.status)
        raise AssertionError("the call reached %s: its check did not fire on the host" % name)


def _poke(pointer, value):
    ctypes.c_int32.from_address(pointer.value).value = value
    return 0


def run(fn, args, kwargs, stand_in, status=None):
    f = getattr(mesh, fn)
    home = sys.modules[f.__module__]
    saved = N.require_cuda, N.lib, N.current_stream, getattr(home, "_staged_call", None)
    try:
        if stand_in:
            N.require_cuda = lambda *t: None
            N.lib = lambda: StandInLibrary(status)
            N.current_stream = lambda: None
        if status is not None:
            home._staged_call = lambda entry, a, stages, times: _poke(a[STATUS_ARG[entry]], status)
        return S.outcome(lambda: f(*args, **kwargs))
    finally:
        N.require_cuda, N.lib, N.current_stream = saved[:3]
        if saved[3] is not None:
            home._staged_call = saved[3]


def main():
    cases = []
    for i, (fn, args, kwargs, wrong) in enumerate(S.CASES):
        exc, msg = run(fn, args, kwargs, wrong != "device")
        assert exc, "%s raised nothing" % S.case_id(i)
        cases.append({"id": S.case_id(i), "exception": exc, "message": msg})
    status = []
    for stage, (args, kwargs, _) in S.STATUS_CALLS.items():
        for bit in S.STATUS_BITS:
            exc, msg = run(stage, args, kwargs, True, status=bit)
            assert exc, "%s raised nothing at status %d" % (stage, bit)
            status.append({"stage": stage, "status": bit, "exception": exc, "message": msg})
    out = {"_comment": "recorded by tests/golden/make_scan_arg_messages.py at the commit before mesh.py was split; see there",
           "cases": cases, "status": status}
    with open(os.path.join(HERE, "scan_arg_messages.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("%d cases, %d status cases" % (len(cases), len(status)))


if __name__ == "__main__":
    main()
