"""A Python MODEL of how the persistent kernels walk their work, written from the kernels' code and comments.  It is not the
kernel: it repeats the walk's integer arithmetic so that a test can say, from the grid a launch reported (rrv_profile_entry_grid),
which items each workgroup ran in which order, and so which boundary code ran between two items.  Plain module, no GPU.

The transform-domain walk (conv_wino_k conv_wino.h:206-233, conv_wino_split_k conv_wino_split.h:70-98, conv_f43_k conv_f43.h:241-271,
the upsample-fused conv_wino_k conv_ups5.h:104-135 — four copies of the same code):
  an item is (tx, ty, b, nt): a pixel tile of image b and one 32-cout slab; pix = (b * tiles_y + ty) * tiles_x + tx.
  xcd_slabs (the host sets it when grid % 8 == 0 and (grid / 8) % slabs == 0, rerevst_hip.hip conv()): workgroup w runs on XCD
    w % 8; PT = grid / 8 / slabs pixel tiles per XCD per round, pix = (w & 7) * PT + (w >> 3) / slabs, nt = (w >> 3) % slabs,
    and a round advances pix by 8 * PT and leaves nt alone;
  plain walk: nt = w % slabs, pix = w / slabs; a round adds grid % slabs to nt (with a carry into the pixel tile) and grid / slabs to pix.
  The kernel divides once, for the first item and for the step (dlt), and then advances (tx, ty, b, nt) with carries; a workgroup
  ends when b reaches B.
Between two items of a chain the kernel re-stages its epilogue parameters when the slab changed, or when the image changed and the
state is per image (conv_wino_split.h:272-276, conv_wino.h:435-438, conv_ups5.h:290-293, conv_f43.h:500-503).

conv_last_k (conv_thin.h:405-414, 431): gridDim % 8 == 0 gives every XCD one contiguous band of ceil(tiles / 8) tiles, which the
grid / 8 workgroups of that XCD take in turn; any other grid walks the tile list round-robin with step grid."""


def host_xcd_slabs(grid, slabs):
    """ConvP::xcd_slabs as conv() sets it."""
    return 1 if grid % 8 == 0 and (grid // 8) % slabs == 0 else 0


def kf_split(H8, W8):
    """The split-K slices of KernelFilter.down_sample for a relu4_1 map of H8 x W8 (rerevst_hip.hip kf_split)."""
    tiles = ((W8 + 15) // 16) * ((H8 + 15) // 16)
    return 8 if tiles * 8 <= 320 else 4 if tiles * 4 <= 512 else 2 if tiles * 2 <= 256 else 1


def td_chain(w, grid, xcd, tiles_x, tiles_y, B, slabs):
    """The items workgroup w of `grid` runs, in order: [(tx, ty, b, nt)].  The kernel's incremental arithmetic, step by step."""
    if xcd:
        PT = (grid >> 3) // slabs
        pix, dpix = (w & 7) * PT + (w >> 3) // slabs, 8 * PT
        nt, dnt = (w >> 3) % slabs, 0
    else:
        nt, pix = w % slabs, w // slabs
        dnt, dpix = grid % slabs, grid // slabs
    tx, ty, b = pix % tiles_x, (pix // tiles_x) % tiles_y, pix // (tiles_x * tiles_y)
    dtx, dty, db = dpix % tiles_x, (dpix // tiles_x) % tiles_y, dpix // (tiles_x * tiles_y)
    out, limit = [], tiles_x * tiles_y * B * slabs + 1
    while b < B:
        out.append((tx, ty, b, nt))
        assert len(out) <= limit, "workgroup %d of %d does not end" % (w, grid)
        nt += dnt
        carry = 0
        if nt >= slabs:
            nt, carry = nt - slabs, 1
        tx += dtx + carry
        if tx >= tiles_x:
            tx, ty = tx - tiles_x, ty + 1
        ty += dty
        if ty >= tiles_y:
            ty, b = ty - tiles_y, b + 1
        b += db
    return out


def td_walk(grid, xcd, tiles_x, tiles_y, B, slabs):
    return [td_chain(w, grid, xcd, tiles_x, tiles_y, B, slabs) for w in range(grid)]


def td_facts(grid, xcd, tiles_x, tiles_y, B, slabs):
    """(longest chain, slab changes inside chains, image changes inside chains) of a launch."""
    longest = slab_changes = image_changes = 0
    for chain in td_walk(grid, xcd, tiles_x, tiles_y, B, slabs):
        longest = max(longest, len(chain))
        for a, c in zip(chain, chain[1:]):
            slab_changes += a[3] != c[3]
            image_changes += a[2] != c[2]
    return longest, slab_changes, image_changes


def td_classes(grid, xcd, tiles_x, tiles_y, B, slabs, per_image):
    """The walk classes a transform-domain launch exercises:
      A  XCD walk, some workgroup runs >= 2 items
      B  plain walk with grid % slabs == 0, some workgroup runs >= 2 items (the slab never changes inside a chain)
      C  plain walk with grid % slabs != 0 and a slab change inside a chain: the kernel re-stages
      I  per-image state and an image change inside a chain (either walk): the kernel re-stages"""
    longest, slab_changes, image_changes = td_facts(grid, xcd, tiles_x, tiles_y, B, slabs)
    out = set()
    if longest >= 2:
        if xcd:
            out.add("A")
        elif grid % slabs == 0:
            out.add("B")
        elif slab_changes:
            out.add("C")
        if per_image and image_changes:
            out.add("I")
    assert not (xcd and slab_changes) and not (grid % slabs == 0 and slab_changes)
    return out


def last_chain(w, grid, ntiles):
    """The tiles workgroup w of conv_last_k runs, in order."""
    if grid & 7 == 0:
        band, xcd = (ntiles + 7) >> 3, w & 7
        tile, step, end = xcd * band + (w >> 3), grid >> 3, min((xcd + 1) * band, ntiles)
    else:
        tile, step, end = w, grid, ntiles
    out = []
    while tile < end:
        out.append(tile)
        tile += step
    return out


def last_walk(grid, ntiles):
    return [last_chain(w, grid, ntiles) for w in range(grid)]


def last_classes(grid, ntiles):
    """'band' / 'rr' (round robin) when some workgroup runs >= 2 tiles in that walk."""
    if max(len(c) for c in last_walk(grid, ntiles)) < 2:
        return set()
    return {"band" if grid & 7 == 0 else "rr"}
