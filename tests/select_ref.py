"""Host reference of the stable class-major selection (k_select_points in csrc/front.hip behind pbn_select_points), written from
the contract in include/pbnet_hip.h.  Numpy, explicit loops, no knowledge of blocks, waves, rounds or ballots.

The contract as this file reads it
  * sem_pred int64 [n] holds a class in [0, n_cls) or a NEGATIVE value; a negative label belongs to no class: the point is not
    selected and takes no position.  Labels >= n_cls are outside the contract (the kernel indexes tables of n_cls words with them).
  * class_base int32 [n_cls]: class_base[c] < 0 drops class c, its points are not selected and take no position; otherwise point i
    of class c goes to position class_base[c] + #{j < i : sem_pred[j] == c}.  Nothing asks class_base to ascend with c: the caller
    only owes disjoint ranges [class_base[c], class_base[c] + population of c).
  * ins_ind[pos] = i, ins_orig[pos] = xyz[i], ins_off[pos] = float32(xyz[i]) + float32(offset[i]) -- ONE float32 addition, whatever
    type the offsets are stored in --, ins_sem[pos] = c.  Positions nobody is sent to are not written.
16-bit offsets are float32 arrays already representable in the type, so widening them on the device is exact."""
import numpy as np

F32 = np.float32


def select_points(sem_pred, class_base, xyz, offset_f32):
    """-> dict(ins_ind int64 [m], ins_orig f32 [m, 3], ins_off f32 [m, 3], ins_sem int32 [m], written bool [m], total) with m = one
    past the highest position written (0 when nothing is selected) and total = the number of selected points."""
    sem_pred = np.asarray(sem_pred, np.int64)
    class_base = np.asarray(class_base, np.int64)
    xyz, off = np.asarray(xyz, F32), np.asarray(offset_f32, F32)
    n, n_cls = sem_pred.shape[0], class_base.shape[0]
    assert xyz.shape == (n, 3) and off.shape == (n, 3) and (sem_pred < n_cls).all()
    seen = [0] * n_cls
    where = []
    for i, c in enumerate(sem_pred.tolist()):
        if c < 0:
            continue
        if class_base[c] >= 0:
            where.append((int(class_base[c]) + seen[c], i, c))
        seen[c] += 1
    m = max(p for p, _, _ in where) + 1 if where else 0
    out = dict(ins_ind=np.zeros(m, np.int64), ins_orig=np.zeros((m, 3), F32), ins_off=np.zeros((m, 3), F32),
               ins_sem=np.zeros(m, np.int32), written=np.zeros(m, bool), total=len(where))
    for p, i, c in where:
        assert not out["written"][p], "class ranges overlap: the caller's class_base is outside the contract"
        out["written"][p] = True
        out["ins_ind"][p], out["ins_sem"][p] = i, c
        out["ins_orig"][p] = xyz[i]
        for a in range(3):
            out["ins_off"][p, a] = F32(xyz[i, a]) + F32(off[i, a])              # one float32 addition
    return out


def block_hist(sem_pred, n_cls, block_rows):
    """int32 [max(blocks, 1), n_cls]: points of class c among the block_rows points of block b -- what pbn_sem_argmax_table leaves
    for pbn_select_points (block_rows = the rows of one pbn_select_blocks block).  Negative labels are in no class."""
    sem_pred = np.asarray(sem_pred, np.int64)
    blocks = -(-sem_pred.shape[0] // block_rows)
    hist = np.zeros((max(blocks, 1), n_cls), np.int32)
    for i, c in enumerate(sem_pred.tolist()):
        if c >= 0:
            hist[i // block_rows, c] += 1
    return hist
