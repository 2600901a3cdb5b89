"""SH layouts off the diagonal: an active degree D below what the M allocated coefficients would hold, and M that is no
square.  The C ABI takes D and M separately and accepts every pair 0 <= D <= 3, (D+1)^2 <= M <= 16 (gsr_forward); what
the per-Gaussian kernels do with SH is selected by M -- which k_preprocess variant, the LDS row stride, the 16-byte or
the scalar copy branches -- while the arithmetic follows D.  synthetic.make_gaussians only builds M = (D+1)^2.

`launch_cells` restates the launch conditions of launch_preprocess / launch_gaussian_backward and of the three SH row
helpers (rows_to_lds, listed_rows_to_lds, lds_to_rows in csrc/preprocess.hip) from what a caller hands in; the GPU cases
assert the cell they are there for and tests/test_sh_layouts.py asserts that their union covers every cell."""
from gs_livm_amd import synthetic as S
import numpy as np

PAIRS = [(D, M) for D in range(4) for M in range((D + 1) ** 2, 17)]                      # the 38 legal pairs
VARIANT_PAIRS = [(0, 16), (1, 16), (2, 16), (0, 4), (0, 9), (1, 9), (1, 8), (2, 12), (0, 2), (1, 7)]
SCALE_PAIRS = [(0, 16), (1, 16), (2, 16), (0, 4), (1, 8)]                                # at 200 003 Gaussians
DEPTH_PAIRS = [(0, 16), (1, 9), (0, 1)]
# (M = 2 admits the active degree 0 only: (1, 2) is no legal pair, the library refuses it -- REFUSED_ALIGN_PAIR is held
# to that refusal instead)
ALIGN_PAIRS = [(3, 16), (1, 4), (0, 16), (1, 8), (2, 9), (0, 2), (0, 1)]
REFUSED_ALIGN_PAIR = (1, 2)
SMALL, MID, TINY, LARGE = (300, 70, 50, 11), (1500, 200, 120, 13), (7, 33, 17, 3), (200_003, 320, 200, 37)
PRE_BLOCK = 256
assert len(PAIRS) == 38 and set(VARIANT_PAIRS) | set(ALIGN_PAIRS) <= set(PAIRS)


def with_layout(P, W, H, seed, D, M):
    """The first M coefficients of make_scene(P, W, H, seed, sh_degree=3), rendered at active degree D."""
    assert (D, M) in PAIRS
    sc = S.make_scene(P, W, H, seed, sh_degree=3)
    sc["shs"] = np.ascontiguousarray(sc["shs"][:, :M])
    sc["sh_degree"] = D
    return sc


def natural_degree(M):
    """The degree a kernel would take if it read it off M: floor(sqrt(M)) - 1."""
    return int(np.floor(np.sqrt(M))) - 1


# ---- which kernel variant and which copy branches a call runs (csrc/preprocess.hip restated) ----------------------
FORWARD_VARIANTS = ("rowk12", "rowk3", "block_copy", "plain", "general")


def _row_class(M):
    c = 3 * M
    return "0mod4" if c % 4 == 0 else "2mod4" if c % 2 == 0 else "odd"


def _copy_branch(M, ptr):
    """(branch, row class) of one SH row helper: 16-byte accesses iff 3M is a multiple of 4 and the base is 16-byte
    aligned (a block's first row is then aligned too: rows of 12M bytes); the LDS stride is 3M | 1, != 3M for even 3M."""
    return ("vec16" if (3 * M) % 4 == 0 and ptr % 16 == 0 else "scalar", _row_class(M))


def launch_cells(P, D, M, debug, shs_ptr=0, dsh_ptr=0, colors_precomp=False, cov3D_precomp=False, depth=False):
    """{forward, shs_full, backward, shs_listed, dL_dsh}: the k_preprocess variant, the branch of rows_to_lds (None
    where it does not run), the k_gaussian_backward instantiation, and the branches of listed_rows_to_lds / lds_to_rows
    (None when the backward is not staged)."""
    sh = not colors_precomp
    stage = sh and M > 1 and PRE_BLOCK * ((3 * M) | 1) * 4 <= 64 * 1024
    plain_in = sh and not cov3D_precomp and not debug
    rows16 = plain_in and shs_ptr % 16 == 0
    if stage and rows16 and M == 16:
        fwd = "rowk12"
    elif stage and rows16 and M == 4:
        fwd = "rowk3"
    elif stage:
        fwd = "block_copy"
    elif D == 0 and plain_in:
        fwd = "plain"
    else:
        fwd = "general"
    # the pipelined variants copy block-wide only their last, partial block
    full = fwd == "block_copy" or (fwd in ("rowk12", "rowk3") and P % PRE_BLOCK != 0)
    cells = dict(forward=fwd, shs_full=_copy_branch(M, shs_ptr) if full else None,
                 backward=("staged" if stage else "unstaged") + ("+depth" if depth else ""))
    cells["shs_listed"] = _copy_branch(M, shs_ptr) if stage else None
    cells["dL_dsh"] = _copy_branch(M, dsh_ptr) if stage else None
    return cells


COPY_CELLS = [("vec16", "0mod4"), ("scalar", "0mod4"), ("scalar", "2mod4"), ("scalar", "odd")]


def required_cells():
    """Every cell the GPU module has to reach (the issue's coverage list)."""
    need = {("forward", v) for v in FORWARD_VARIANTS}
    need |= {("forward@D", "rowk12", D) for D in range(4)} | {("forward@D", "rowk3", D) for D in range(2)}
    need |= {("backward", s + d) for s in ("staged", "unstaged") for d in ("", "+depth")}
    need |= {(h,) + c for h in ("shs_full", "shs_listed", "dL_dsh") for c in COPY_CELLS}
    return need


def cells_reached(cells, D):
    got = {("forward", cells["forward"]), ("backward", cells["backward"])}
    if cells["forward"] in ("rowk12", "rowk3"):
        got.add(("forward@D", cells["forward"], D))
    for h in ("shs_full", "shs_listed", "dL_dsh"):
        if cells[h] is not None:
            got.add((h,) + cells[h])
    return got


# ---- the GPU module's cases, stated here so that the coverage test needs no GPU ------------------------------------
# alignment placements: byte offset (mod 16) of every Arena view, by tensor name
def placement(mode):
    """all at 4 / 8 / 12 ("a4" ...), cycling ("mix"), or one tensor (group) at 8 bytes and the rest aligned
    ("only:shs", "only:dL_dsh", "only:means3D", "only:images").  `rotations` stays 16-byte aligned throughout: the
    contract (include/gsraster.h)."""
    images = ("out_color", "out_depth", "out_acc")

    def off(name, _i=None):   # (by the tensor's place in ARENA_ORDER, whatever else the arena holds)
        i = ARENA_ORDER.index(name)
        if name in ("rotations", "cov3D_precomp") and mode == "mix":
            return (0, 12)[name != "rotations"]
        if name == "rotations":
            return 0
        if mode == "mix":
            return (4, 8, 12, 0)[i % 4]
        if mode.startswith("only:"):
            grp = mode[5:]
            return 8 if name == grp or (grp == "images" and name in images) else 0
        return int(mode[1:])
    return off


PLACEMENTS = ("a4", "a8", "a12", "mix", "only:shs", "only:dL_dsh", "only:means3D", "only:images")
# the order in which the alignment test puts its tensors into the arena ("mix" cycles through 0/4/8/12 in this order)
ARENA_ORDER = ("means3D", "scales", "rotations", "opacities", "shs", "colors_precomp", "cov3D_precomp", "viewmatrix", "projmatrix", "campos", "bg",
               "out_color", "out_depth", "out_acc", "radii", "dL_dpix", "dL_dacc", "dL_ddepth", "dL_dmeans2D",
               "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
               "dL_drotations", "dL_ddepths")


def placed_offset(mode, name):
    return placement(mode)(name)


def gpu_cases():
    """(what, P, D, M, kwargs of launch_cells) of every forward / backward the GPU module runs with SH."""
    out = []
    for D, M in PAIRS:                      # items 1 and 2: debug and product passes, allocator-aligned tensors
        for debug in (True, False):
            out.append(("pairs", SMALL[0], D, M, dict(debug=debug)))
    for D, M in VARIANT_PAIRS:              # items 1-4 at 1 500: the last block (220 rows) is partial
        for debug in (True, False):
            out.append(("variants", MID[0], D, M, dict(debug=debug)))
    for D, M in DEPTH_PAIRS:
        out.append(("depth", SMALL[0], D, M, dict(debug=False, depth=True)))
    for D, M in SCALE_PAIRS:
        for debug in (True, False):
            out.append(("scale", LARGE[0], D, M, dict(debug=debug)))
    for D, M in ALIGN_PAIRS:
        for mode in PLACEMENTS:
            out.append(("align:" + mode, SMALL[0], D, M,
                        dict(debug=False, depth=True, shs_ptr=placed_offset(mode, "shs"),
                             dsh_ptr=placed_offset(mode, "dL_dsh"))))
    out.append(("align:colors_precomp", SMALL[0], 0, 1, dict(debug=False, depth=True, colors_precomp=True)))
    out.append(("align:cov3D_precomp", SMALL[0], 1, 8, dict(debug=False, depth=True, cov3D_precomp=True,
                                                             shs_ptr=placed_offset("mix", "shs"),
                                                             dsh_ptr=placed_offset("mix", "dL_dsh"))))
    return out
