"""The launch arithmetic of the position-major split-precision weight gradient (csrc/kws_cnn_shape.h: WgradPm, wgrad_pm_plan; csrc/kws_conv.h: the block
decoding at the top of conv_wgrad_bf16_kernel<..., PM = true>), restated in Python, and the feature maps the tests use.

conv4 (3 x 3, stride 1, 'same') maps the H3 x W3 map conv3 (3 x 3, stride 2, 'same') produces onto itself.  When that map has at most 16
pixels, conv4's weight gradient in a split-precision, non-deterministic train step (csrc/kws_cnn_plan.h: wgrad_pmajor) reduces over
(output position, clip): a chunk is 32 clips at ONE output position, so a (tap, position) pair is either inside the input map for
the whole chunk or in the padding for the whole chunk, and padding pairs are never staged or multiplied.  (conv3's weight gradient
keeps the pixel-major kernel: its kernel-row form of the same idea measured slower)  The restatement keeps the
general form -- any stride and padding, `tpb` taps per group -- and the library uses it with one tap per group.

    lists      a tap group is `tpb` consecutive taps (the library: one).  It keeps the positions at which at least one of its taps
               reads inside the map, with the mask of those taps; its weight is its number of (tap, position) products.
    clips      the NC = ceil(B / 32) clip chunks are dealt to the 8 XCDs: XCD x takes [x NC // 8, (x + 1) NC // 8) for EVERY group, so
               the groups reading one clip range share an L2.
    slots      an XCD has S block slots (block id = 8 slot + x): S = ceil(positions NC / (8 min_chunks)), at least one per group with
               products, at most max_slots = CUs * resident blocks // 8 (one resident round).  Group g starts at floor(S w_g / sum w)
               slots (at least 1); the slots left go one by one to the group with the most products per slot (lowest index on ties);
               slots too many leave the group with the fewest (highest index on ties).
    items      inside (XCD, group) the items are (clip chunk major, kept position minor); slot k of the group's n takes items
               k, k + n, k + 2 n, ...: slots per group follow items per group, so all blocks of an XCD are at about the same clip
               chunk at the same time and the groups find each other's rows in the L2.

The bound this rule implies: the blocks of one (XCD, group) differ by at most one chunk, the XCDs' clip ranges by at most one chunk,
and a group's slots differ from its exact share S w_g / sum w by less than one whenever that share is at least one (a group receives at
most one slot beyond the floor of its share: once it has it, its products per slot are below the average sum w / S, and while slots
are left some group is above it)."""
import collections

MI355X_CUS = 256
RESIDENT = 3                        # blocks per CU of conv4's instantiation: 138 registers, 43008 bytes of LDS
MAX_SLOTS = MI355X_CUS * RESIDENT // 8
CLIPS = 32                          # clips per chunk

Layer = collections.namedtuple("Layer", "name H W Ho Wo stride pt pl tpb min_chunks")
Plan = collections.namedtuple("Plan", "pos taps weight slot0")

# (frames, coefficients) -> what it is here for
MAPS = collections.OrderedDict((
    ((30, 20), "the default map: a2 7 x 5, conv3 pads one row / column on every side, 4 x 3 outputs"),
    ((32, 24), "a2 8 x 6 is even: conv3 pads bottom and right only (pt = pl = 0), 4 x 3 outputs"),
    ((26, 18), "a2 6 x 4 -> 3 x 2 outputs: a small non-square map with an odd side"),
    ((30, 30), "a2 7 x 7 -> 4 x 4 outputs: exactly 16 pixels"),
    ((30, 40), "a2 7 x 10 -> 4 x 5 outputs: 20 pixels, the pixel-major kernel stays"),
))
ONE_SIDED, ODD, SIXTEEN, FALLBACK = (32, 24), (26, 18), (30, 30), (30, 40)


def same_out(n, s):
    return (n + s - 1) // s


def same_pad_before(n, k, s):
    return max((same_out(n, s) - 1) * s + k - n, 0) // 2


def layers(nf, fs):
    """the position-major launch of a map: conv4 over a3, one tap per block.  conv3's geometry (over a2, stride 2, one kernel row per
    group) rides along for the arithmetic only: it is where padding can sit on one side (an even a2)"""
    H2, W2 = nf // 2 // 2, fs // 2 // 2
    H3, W3 = same_out(H2, 2), same_out(W2, 2)
    return (Layer("conv3-geometry", H2, W2, H3, W3, 2, same_pad_before(H2, 3, 2), same_pad_before(W2, 3, 2), 3, 2),
            Layer("conv4", H3, W3, H3, W3, 1, 1, 1, 1, 4))


def applies(nf, fs):
    """csrc/kws_cnn_plan.h: wgrad_pmajor (split precision, training, not deterministic)"""
    lay = layers(nf, fs)[1]
    return lay.Ho * lay.Wo <= 16


def inside(lay, tap, p):
    kh, kw = divmod(tap, 3)
    oy, ox = divmod(p, lay.Wo)
    sy, sx = oy * lay.stride + kh - lay.pt, ox * lay.stride + kw - lay.pl
    return 0 <= sy < lay.H and 0 <= sx < lay.W


def plan(lay, B, max_slots=MAX_SLOTS):
    """wgrad_pm_plan: per group the kept positions, their tap masks, the weight, and the groups' first slots"""
    ngroups = 9 // lay.tpb
    pos, taps, w = [], [], []
    for g in range(ngroups):
        ps, ms = [], []
        for p in range(lay.Ho * lay.Wo):
            mask = sum(1 << t for t in range(lay.tpb) if inside(lay, g * lay.tpb + t, p))
            if mask:
                ps.append(p)
                ms.append(mask)
        pos.append(ps)
        taps.append(ms)
        w.append(sum(bin(m).count("1") for m in ms))
    live = sum(1 for x in w if x)
    assert 1 <= live <= max_slots
    nclip = (B + CLIPS - 1) // CLIPS
    want = -(-sum(len(p) for p in pos) * nclip // (8 * lay.min_chunks))
    S = min(max(want, live), max_slots)
    s = [max(1, S * x // sum(w)) if x else 0 for x in w]
    while sum(s) < S:
        best = -1
        for g in range(ngroups):
            if w[g] and (best < 0 or w[g] * s[best] > w[best] * s[g]):
                best = g
        s[best] += 1
    while sum(s) > S:
        best = -1
        for g in range(ngroups):
            if s[g] > 1 and (best < 0 or w[g] * s[best] <= w[best] * s[g]):
                best = g
        s[best] -= 1
    slot0 = [0]
    for n in s:
        slot0.append(slot0[-1] + n)
    return Plan(pos, taps, w, slot0)


def grid(pl):
    return 8 * pl.slot0[-1]


def block_items(lay, pl, B, bid):
    """the kernel's decoding of a block id -> (group, [(clip chunk, position, tap mask), ...])"""
    ngroups = 9 // lay.tpb
    xcd, slot = bid & 7, bid >> 3
    g = 0
    while g + 1 < ngroups and slot >= pl.slot0[g + 1]:
        g += 1
    nclip = (B + CLIPS - 1) // CLIPS
    c0, c1 = xcd * nclip // 8, (xcd + 1) * nclip // 8
    k, ns, npos = slot - pl.slot0[g], pl.slot0[g + 1] - pl.slot0[g], len(pl.pos[g])
    if not (k < ns and npos):
        return g, []
    items = (c1 - c0) * npos
    return g, [(c0 + i // npos, pl.pos[g][i % npos], pl.taps[g][i % npos]) for i in range(k, items, ns)]


def full_round_batch(lay, lo=1, hi=4096):
    """the first B at which the launch fills the resident round (8 * MAX_SLOTS blocks) and every block has a chunk"""
    for B in range(lo, hi):
        pl = plan(lay, B)
        if grid(pl) == 8 * MAX_SLOTS and all(block_items(lay, pl, B, b)[1] for b in range(grid(pl))):
            return B
    return None


# The GPU cases' two larger batches on the default map, from the arithmetic above (tests/test_wgrad_pmajor_host.py checks them):
# B = 1377 is the first batch at which conv4's launch is one full resident round of 768 blocks, every one with work (70 kept
# (tap, position) pairs * 44 clip chunks >= 4 chunks * 767 blocks); at B = 1399 the same grid holds blocks of 3, 4 and 5 chunks and
# the last chunk of every position has 23 clips.
B_FULL, B_UNEQUAL = 1377, 1399
