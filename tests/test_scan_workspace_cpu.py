"""CPU tier: the workspace sizes of the scan-decode chain (csrc/mesh.hip, cloud.hip, thin.hip, vote.hip) are pinned.  The
stages carve their sort buffers through one helper (csrc/sort_dev.h); a change of its order or sizes would move every
pbn_*_workspace_bytes below.  The tables were recorded from the library as it was before the stages shared that helper, and
are literals on purpose: nothing here is computed from the code under test.  The functions run on the host alone."""
import pytest

from pbnet_amd import _native as N

SIZES = (0, 1, 255, 256, 257, 2049, 100000)      # around the 256-byte carve, a block of 256 and a scan tile of 2048
KS = (1, 32)
MODES = (0, 1, 2)                                # normals, segment, segment_point
OVER = (1 << 28) + 1                             # one more point than the chain takes

# [n][k]
CLOUD = (
    84224, 84224, 84224, 84224, 93184, 93184, 93184, 93184, 94464, 94464, 223520, 223520, 8430080, 8430080,
)
# [n]
THIN = (
    76300, 76300, 84748, 84748, 86540, 182800, 5254860,
)
OUTLIER = (
    1028, 1028, 2820, 2820, 3336, 19492, 905244,
)
RAW_INDEX = (
    780, 780, 2316, 2316, 2828, 17168, 800716,
)
# [n_raw][m]
VOTE = (
    16857604, 16857604, 16857604, 16857604, 16857604, 16857604, 16857604, 16857604, 16857604, 16857604, 16857604,
    16857604, 16857604, 16857604, 16865028, 16865028, 16865028, 16865028, 16865028, 16865028, 16865028, 16865028,
    16865028, 16865028, 16865028, 16865028, 16865028, 16865028, 16866820, 16866820, 16866820, 16866820, 16866820,
    16866820, 16866820, 16955908, 16955908, 16955908, 16955908, 16955908, 16955908, 16955908, 21636100, 21636100,
    21636100, 21636100, 21636100, 21636100, 21636100,
)
# [mode][n_vertices][n_elems]
MESH = (
    2060, 2060, 10508, 11020, 11276, 75788, 3601676, 2060, 2060, 10508, 11020, 11276, 75788, 3601676, 4364, 4364, 12812,
    13324, 13580, 78092, 3603980, 4620, 4620, 13068, 13580, 13836, 78348, 3604236, 5132, 5132, 13580, 14092, 14348,
    78860, 3604748, 26640, 26640, 35088, 35600, 35856, 100368, 3626256, 1201868, 1201868, 1210316, 1210828, 1211084,
    1275596, 4801484, 54024, 54024, 94472, 95240, 97032, 471816, 20440584, 54024, 54024, 94472, 95240, 97032, 471816,
    20440584, 60928, 60928, 101376, 102144, 103936, 478720, 20447488, 61188, 61188, 101636, 102404, 104196, 478980,
    20447748, 62216, 62216, 102664, 103432, 105224, 480008, 20448776, 119560, 119560, 160008, 160776, 162568, 537352,
    20506120, 3253380, 3253380, 3293828, 3294596, 3296388, 3671172, 23639940, 52232, 52232, 62728, 62728, 64520, 175112,
    6030600, 52232, 52232, 62728, 62728, 64520, 175112, 6030600, 54016, 54016, 64512, 64512, 66304, 176896, 6032384,
    54020, 54020, 64516, 64516, 66308, 176900, 6032388, 54280, 54280, 64776, 64776, 66568, 177160, 6032648, 68616,
    68616, 79112, 79112, 80904, 191496, 6046984, 852100, 852100, 862596, 862596, 864388, 974980, 6830468,
)


def _expect(table, *index):
    """table is row-major over `index` = (position, length) pairs"""
    at = 0
    for pos, length in index:
        at = at * length + pos
    return table[at]


@pytest.mark.parametrize("i", range(len(SIZES)))
def test_workspace_bytes_of_one_size(i):
    lib, n = N.lib(), SIZES[i]
    for j, k in enumerate(KS):
        assert lib.pbn_cloud_workspace_bytes(n, k) == _expect(CLOUD, (i, len(SIZES)), (j, len(KS))), (n, k)
    assert lib.pbn_thin_workspace_bytes(n) == THIN[i], n
    assert lib.pbn_cloud_outlier_workspace_bytes(n) == OUTLIER[i], n
    assert lib.pbn_cloud_raw_index_workspace_bytes(n) == RAW_INDEX[i], n


@pytest.mark.parametrize("i", range(len(SIZES)))
def test_workspace_bytes_of_two_sizes(i):
    lib, n = N.lib(), SIZES[i]
    for j, m in enumerate(SIZES):
        assert lib.pbn_cloud_vote_workspace_bytes(n, m) == _expect(VOTE, (i, len(SIZES)), (j, len(SIZES))), (n, m)
        for mode in MODES:
            want = _expect(MESH, (mode, len(MODES)), (i, len(SIZES)), (j, len(SIZES)))
            assert lib.pbn_mesh_workspace_bytes(mode, n, m) == want, (mode, n, m)


def test_workspace_refusals():
    lib = N.lib()
    assert lib.pbn_cloud_workspace_bytes(1 << 28, 1) > 0
    assert lib.pbn_cloud_workspace_bytes(OVER, 1) == 0
    assert lib.pbn_cloud_workspace_bytes(256, 33) == 0 and lib.pbn_cloud_workspace_bytes(256, 0) == 0
    assert lib.pbn_cloud_workspace_bytes(-1, 1) == 0
    assert lib.pbn_thin_workspace_bytes(OVER) == 0
    assert lib.pbn_cloud_outlier_workspace_bytes(OVER) == 0
    assert lib.pbn_cloud_raw_index_workspace_bytes(OVER) == 0
    assert lib.pbn_cloud_vote_workspace_bytes(OVER, 1) == 0 and lib.pbn_cloud_vote_workspace_bytes(1, OVER) == 0
    # a mesh counts edges: 2^30 - 1 of them at the most, three per face
    assert lib.pbn_mesh_workspace_bytes(2, 1, (1 << 30) - 1) > 0 and lib.pbn_mesh_workspace_bytes(2, 1, 1 << 30) == 0
    assert lib.pbn_mesh_workspace_bytes(0, 1, ((1 << 30) - 1) // 3) > 0
    assert lib.pbn_mesh_workspace_bytes(1, 1, ((1 << 30) - 1) // 3 + 1) == 0
    assert lib.pbn_mesh_workspace_bytes(3, 1, 1) == 0 and lib.pbn_mesh_workspace_bytes(-1, 1, 1) == 0
    assert lib.pbn_mesh_workspace_bytes(0, -1, 1) == 0
