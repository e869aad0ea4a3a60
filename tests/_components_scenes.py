"""Constructed depth images for the connected-component tests.  A pixel is a depth in metres (float32), 0 = invalid.  At
NEAR, neighbouring pixels lie under 2 mm apart (the diagonal included), far inside the default tolerance of 10 mm, so
validity alone decides the components; NEAR and FAR are 10 cm apart, so the distance test cuts between them.  Nothing here
knows the kernel's tile size: the seam scenes hit every column, row and corner boundary."""
import numpy as np

F = np.float32
NEAR, FAR = F(0.5), F(0.6)
K = np.array([[600.0, 0.0, 64.5], [0.0, 600.0, 32.5], [0.0, 0.0, 1.0]], F)


def to_raw16(depth):
    """The raw 16-bit encoding pgp_backproject_depth reads (rotate right by 3 undone): metres, in 0.1 mm steps."""
    s = np.rint(np.asarray(depth, np.float64) * 10000.0).astype(np.uint32) & 0xFFFF
    return (((s << 3) | (s >> 13)) & 0xFFFF).astype(np.uint16)


def flat(rows, cols, depth=NEAR):
    return np.full((rows, cols), depth, F)


def from_valid(valid, depth=NEAR):
    return np.where(valid, depth, F(0)).astype(F)


def column_seams(cols=130, phase=0):
    """3 x cols: rows 0 and 2 hold two-pixel components whose depths alternate (the distance test cuts between pairs); row 0
    straddles the odd column boundaries, row 2 the even ones, row 1 is invalid.  `phase` swaps the rows."""
    img = np.zeros((3, cols), F)
    for row, off in ((0, phase), (2, 1 - phase)):
        c = np.arange(cols)
        pair = (c + off) // 2
        img[row] = np.where(pair % 2 == 0, NEAR, FAR)
    return img


def row_seams(rows=130, phase=0):
    return np.ascontiguousarray(column_seams(rows, phase).T)


def diagonal_pairs(n=66, anti=False, phase=0):
    """n x n: two-pixel components joined by a diagonal step only, along the main diagonal (or the anti-diagonal), depths
    alternating from pair to pair; phases 0 and 1 together put a pair across every (r, c) -> (r + 1, c + 1) of the diagonal."""
    img = np.zeros((n, n), F)
    for r in range(n):
        c = n - 1 - r if anti else r
        img[r, c] = NEAR if ((r + phase) // 2) % 2 == 0 else FAR
    return img


def spiral(rows=65, cols=129):
    """A one-pixel-wide corridor spiralling inwards from (0, 0), walls one pixel wide: one component, root 0."""
    v = np.zeros((rows, cols), bool)
    v[0, 0] = True
    r, c, d = 0, 0, 0
    dirs = ((0, 1), (1, 0), (0, -1), (-1, 0))

    def inside(a, b):
        return 0 <= a < rows and 0 <= b < cols

    def free(dr, dc):   # the next cell is new and touches nothing but the cell we stand on
        nr, nc = r + dr, c + dc
        if not inside(nr, nc) or v[nr, nc]:
            return False
        near = ((nr + dr, nc + dc), (nr + dc, nc + dr), (nr - dc, nc - dr))
        return not any(inside(a, b) and v[a, b] for a, b in near)

    while True:
        if not free(*dirs[d]):
            d = (d + 1) % 4
            if not free(*dirs[d]):
                break
        r, c = r + dirs[d][0], c + dirs[d][1]
        v[r, c] = True
    return from_valid(v)


def comb(rows=40, cols=150):
    """Teeth in every other column, joined only along the bottom row: the root is the top of the first tooth."""
    v = np.zeros((rows, cols), bool)
    v[:, ::2] = True
    v[rows - 1, :] = True
    return from_valid(v)


def u_shape(rows=40, cols=200, left=5, right=190):
    """Two arms far apart (different tiles, whatever the tile), joined along the bottom row."""
    v = np.zeros((rows, cols), bool)
    v[:, left] = True
    v[:, right] = True
    v[rows - 1, left:right + 1] = True
    return from_valid(v)


def checkerboard(rows=37, cols=53):
    u, v = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    return from_valid((u + v) % 2 == 0)


def striped_rows(rows=37, cols=53):
    """Every pixel valid, rows alternate between NEAR and FAR: the components are the rows."""
    img = flat(rows, cols)
    img[1::2] = FAR
    return img


def striped_cols(rows=37, cols=53):
    return np.ascontiguousarray(striped_rows(cols, rows).T)


def random_valid(rows=65, cols=129, density=0.59, seed=0):
    rng = np.random.default_rng(seed)
    return from_valid(rng.random((rows, cols)) < density)


def random_levels(rows=65, cols=129, seed=0):
    """Every pixel valid, NEAR or FAR at random: the distance test cuts, validity does not."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((rows, cols)) < 0.55, NEAR, FAR).astype(F)


def blobs(rows=48, cols=96):
    """Four rectangles of 60, 60, 35 and 24 pixels (two of equal size) and a 3-pixel speck: the ranking scene."""
    v = np.zeros((rows, cols), bool)
    v[2:8, 70:80] = True       # 60 pixels, root 2 * cols + 70
    v[20:30, 3:9] = True       # 60 pixels, the larger root
    v[12:17, 40:47] = True     # 35
    v[40:44, 60:66] = True     # 24
    v[45, 90:93] = True        # 3
    return from_valid(v)


def small_scenes():
    """(name, image) of the scenes small enough for a Python flood fill."""
    out = [("flat", flat(5, 7)), ("one", flat(1, 1)), ("row", flat(1, 40)), ("col", flat(40, 1)),
           ("checker", checkerboard(9, 11)), ("rows", striped_rows(8, 9)), ("cols", striped_cols(8, 9)),
           ("spiral", spiral(17, 23)), ("comb", comb(9, 21)), ("u", u_shape(9, 30, 2, 27)),
           ("colseam", column_seams(20)), ("diag", diagonal_pairs(12)), ("anti", diagonal_pairs(12, anti=True, phase=1)),
           ("blobs", blobs())]
    out += [(f"random{s}", random_valid(21, 33, seed=s)) for s in range(3)]
    out += [("levels", random_levels(21, 33, seed=4))]
    return out
