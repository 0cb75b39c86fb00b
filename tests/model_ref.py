"""What tests/test_step_table.py and tests/test_dev_model.py share: the float64
restatement of the model's frames (the chained lookups) and the 1-ulp bar."""
import numpy as np

# the step table's capacities, constants and records (csrc/step_table.h)
NB, NV, NP, NJ, NEQ = 32, 32, 768, 32, 8
MINVAL, MINIMP, MAXIMP = np.float32(1e-15), np.float32(0.0001), np.float32(0.9999)
ANCHOR0, POW2, POW1, LIMITED, CONDIM1 = 1, 1, 2, 4, 8
FREE, BALL, SLIDE, HINGE = 0, 1, 2, 3
BK_FREE, BK_HINGE, BK_SLIDE, BK_WELD = 1, 2, 3, 4
f4, i4 = np.float32, np.int32

BODY = np.dtype([("kind", i4), ("anc", i4), ("qposadr", i4), ("qpos0", f4), ("bquat", f4, 4), ("bpos", f4, 3),
                 ("pad0", f4), ("axis", f4, 3), ("pad1", f4), ("ipos", f4, 3), ("pad2", f4), ("jpos", f4, 3),
                 ("pad3", f4), ("R", f4, (3, 4))])
DOF = np.dtype([("body", i4), ("kind", i4), ("tree", i4), ("sub", i4), ("axis", f4, 3), ("pad0", f4), ("jpos", f4, 3),
                ("pad1", f4)])
ROW = np.dtype([("dmin", f4), ("dmax", f4), ("iwidth", f4), ("mid", f4), ("imid", f4), ("i1mid", f4), ("K", f4),
                ("B", f4), ("margin", f4), ("diag", f4), ("flags", i4), ("power", f4), ("range", f4, 2),
                ("qposadr", i4), ("dofadr", i4)])
TABLE = np.dtype([("flags", i4), ("nbody", i4), ("pad", i4, 2), ("body", BODY, NB), ("dof", DOF, NV),
                  ("row", ROW, NP + NJ + NEQ)])


def close(got, ref, what):
    """got (fp32) within 1 fp32 ulp of ref (float64 formula)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    fin = np.isfinite(ref)
    assert np.array_equal(got[~fin], ref[~fin]), what
    with np.errstate(over="ignore"):
        ulp = np.spacing(np.abs(ref[fin]).astype(np.float32)).astype(np.float64)
    ulp = np.where(np.isfinite(ulp), ulp, np.inf)
    err = np.abs(got[fin] - ref[fin])
    assert (err <= ulp).all(), (what, float((err / ulp).max()))


def qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1],
                     a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def q2m(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def frames(m):
    """Moving-body indices, static world poses, tree indices: the chained lookups."""
    nb = int(m.nbody)
    moving = [b for b in range(1, nb) if m.body_weldid[b] != 0]
    dmap = {b: i for i, b in enumerate(moving)}
    wpos, wquat = np.zeros((nb, 3)), np.zeros((nb, 4))
    wquat[0, 0] = 1
    for b in range(1, nb):
        if b in dmap:
            continue
        p = int(m.body_parentid[b])
        wpos[b] = wpos[p] + q2m(wquat[p]) @ np.asarray(m.body_pos[b], np.float64)
        q = qmul(wquat[p], np.asarray(m.body_quat[b], np.float64))
        wquat[b] = q / np.sqrt((q * q).sum())
    roots = []
    tree = {}
    for b in moving:
        r = int(m.body_rootid[b])
        if r not in roots:
            roots.append(r)
        tree[b] = roots.index(r)
    return moving, dmap, wpos, wquat, tree
