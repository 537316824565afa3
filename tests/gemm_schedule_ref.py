"""The integer rules by which the conv GEMM (csrc/conv_gemm.hip) and the pixel-split weight gradient (csrc/conv_wgrad.hip) cut
their work (csrc/conv_plan.hpp holds them), restated in plain Python from the source, and a simulator that walks every block of a launch through them.

Two halves that the kernels must keep in agreement:
  host rules   -- which schedule a shape gets, the split-K tail plan, the weight gradient's split count and workspace;
  device maps  -- block id -> (tile, K-steps) for the three GEMM schedules, block id -> (m tile, k tile, pixel range) for the
                  weight gradient, and who deposits into / consumes which hand-off slot.

Plain helper module (no torch, no GPU): test_gemm_schedule_cpu.py checks the properties of these rules,
test_gpu_gemm_schedule_rules.py ties the host half to the shipped library, test_gpu_conv_schedules_exact.py runs the kernels on
the plans this model says its cases reach."""
from functools import lru_cache

NUM_CU = 256                    # chip.hpp: kNumCu
NUM_XCD = 8                     # chip.hpp: kNumXcd
BK = 16                         # conv_plan.hpp: kBK, the K-step of the forward / data-gradient GEMM
TILE = 128                      # rows and pixels of the tile every hand-off schedule runs on
SK_WORKERS_PER_CU = 3           # conv_plan.hpp: kSkWorkersPerCu
SK_SLOTS = NUM_CU * SK_WORKERS_PER_CU      # 768: deposit / flag slots of a stream-K launch (kSkWorkers)
TILE_SLOTS = NUM_CU * 4         # 1024: resident blocks of the tile-per-block kernel (kTileSlots)
TAIL_SLOTS = 2048               # deposit / flag slots of the split-K tail (kTailSlots)
SLOT_BYTES = TILE * TILE * 4    # one deposit: ACC_REGS * kThreads * 4 = 65536
WG_PIX = 32                     # conv_plan.hpp: kWgPix, pixels per K-step of the weight gradient
MIN_PIX = 256                   # conv_plan.hpp: kWgMinPix, fewest pixels per split
WG_SLOTS = NUM_CU * 3           # resident weight-gradient blocks
MAX_SPLIT = 8                   # tail_plan: at most 8 K-ranges per tail tile
MIN_STEPS = 8                   # tail_plan: at least 8 K-steps per piece
OVERHEAD = 6.0                  # tail_plan: a piece's fixed cost in K-steps


def ceil_div(a, b):
    return (a + b - 1) // b


def round_up_xcd(n):
    return ceil_div(n, NUM_XCD) * NUM_XCD


# ----------------------------------------------------------------------------------------------
# host rules
# ----------------------------------------------------------------------------------------------
def clamp_reserved(n):
    """runtime.hip: 0 .. half the CUs, rounded up to whole CUs per XCD."""
    n = max(0, min(int(n), NUM_CU // 2))
    return ceil_div(n, NUM_XCD) * NUM_XCD


def sk_workers(reserved):
    return (NUM_CU - reserved) * SK_WORKERS_PER_CU


def want_streamk(tiles, k_steps, reserved):
    """conv_gemm.hip (on a device with all 256 CUs): the persistent schedule for long contractions whose tile count fills the last
    round of resident blocks badly."""
    if tiles * k_steps < sk_workers(reserved):
        return False
    resident = (NUM_CU - reserved) * 3
    rounds = ceil_div(tiles, resident)
    eff = float(tiles) / (float(rounds) * resident)
    return eff < 0.93 if k_steps >= 64 else (k_steps >= 16 and eff < 0.6)


def tail_plan(m_tiles, n_tiles, k_steps, reserved):
    """(split, lead_n): K-ranges per tail tile (0 = no tail) and the pixel tiles of the leading whole rounds."""
    tiles = m_tiles * n_tiles
    if not want_streamk(tiles, k_steps, reserved):
        return 0, 0
    lead_n = (tiles // TILE_SLOTS) * TILE_SLOTS // m_tiles
    if lead_n <= 0 or lead_n >= n_tiles:
        return 0, lead_n
    R = (n_tiles - lead_n) * m_tiles
    best, best_cost = 0, 0.0
    sp = 1
    while sp <= MAX_SPLIT and sp * MIN_STEPS <= k_steps:
        if R * (sp - 1) > TAIL_SLOTS:
            break
        rounds = ceil_div(R * sp, TILE_SLOTS)
        cost = rounds * (float(k_steps) / sp + OVERHEAD)
        if best == 0 or cost < best_cost - 1e-9:
            best, best_cost = sp, cost
        sp += 1
    return best, lead_n


def conv_mpad(M):
    return ceil_div(M, 128) * 128 if M > 64 else (64 if M > 32 else 32)


def conv_kpad(K):
    return ceil_div(K, 128) * 128


def pick_bm(Mpad):
    return 128 if Mpad % 128 == 0 else (64 if Mpad % 64 == 0 else 32)


def gemm_tiles(Nb, OH, OW, M, K):
    """(m_tiles, n_tiles, KT) of the 128 x 128 tile."""
    return ceil_div(M, TILE), ceil_div(Nb * OH * OW, TILE), ceil_div(K, BK)


def gemm_schedule(Nb, OH, OW, M, K, reserved):
    """dasac_conv_gemm_schedule: 1 when the shape's own schedule is stream-K."""
    if pick_bm(conv_mpad(M)) != 128:
        return 0
    m_tiles, n_tiles, KT = gemm_tiles(Nb, OH, OW, M, K)
    return 1 if want_streamk(m_tiles * n_tiles, KT, reserved) else 0


def gemm_tail_split(Nb, OH, OW, M, K, reserved):
    """dasac_conv_gemm_tail_split."""
    if pick_bm(conv_mpad(M)) != 128:
        return 0
    return tail_plan(*gemm_tiles(Nb, OH, OW, M, K), reserved)[0]


def gemm_workspace():
    """dasac_conv_gemm_workspace: a deposit per slot of the larger schedule, then kTailSlots + 1 flags."""
    return max(TAIL_SLOTS, SK_SLOTS) * SLOT_BYTES + (TAIL_SLOTS + 1) * 4


def wgrad_bn(Cx):
    return 64 if (Cx % 128 != 0 and Cx % 64 == 0) else 128


@lru_cache(maxsize=None)
def fill_rounds(tiles, max_splits, slots):
    """The split count in 1 .. max_splits whose blocks fill whole rounds best; fewer splits unless clearly (2 %) better."""
    best, best_eff = 1, 0.0
    for sp in range(1, max_splits + 1):
        blocks = tiles * sp
        rounds = ceil_div(blocks, slots)
        eff = float(blocks) / (float(rounds) * slots)
        if eff > best_eff + 0.02:
            best_eff, best = eff, sp
    return best


def wgrad_cap(tiles, Npix):
    return ceil_div(WG_SLOTS, tiles) if (tiles < 12 and Npix >= 200000) else 64


def wgrad_splits(Mpad, Kpad, Npix, bm, bnk=128):
    tiles = (Mpad // bm) * (Kpad // bnk)
    max_splits = min(ceil_div(Npix, MIN_PIX), wgrad_cap(tiles, Npix))
    return fill_rounds(tiles, max_splits, WG_SLOTS)


def wgrad_per(Npix, splits):
    """Pixels per split: an equal share rounded UP to whole 32-pixel steps, so trailing splits can start at or past Npix."""
    return ceil_div(ceil_div(Npix, splits), WG_PIX) * WG_PIX


def wgrad_layout(M, K, Cx, Npix):
    """(Mpad, Kpad, bm, bnk, splits) of a weight-gradient launch (WgradLayout)."""
    Mpad, Kpad = conv_mpad(M), conv_kpad(K)
    bm = pick_bm(Mpad)
    bnk = wgrad_bn(Cx) if (M % 8 == 0 and bm != 32) else 128
    return Mpad, Kpad, bm, bnk, wgrad_splits(Mpad, Kpad, Npix, bm, bnk)


def wgrad_workspace(Nb, OH, OW, M, K):
    """dasac_conv_wgrad_workspace: slabs + per-split channel sums at the larger split count of both k-tile widths."""
    Mpad, Kpad = conv_mpad(M), conv_kpad(K)
    bm = pick_bm(Mpad)
    splits = max(wgrad_splits(Mpad, Kpad, Nb * OH * OW, bm, 128), wgrad_splits(Mpad, Kpad, Nb * OH * OW, bm, 64))
    return splits * Mpad * (Kpad + 1) * 4


# ----------------------------------------------------------------------------------------------
# device maps: the GEMM
# ----------------------------------------------------------------------------------------------
def _block(bid):
    # segments: (tile, ks, ke) in launch order; deposit: the slot written (a non-owner); consumes: slots waited for and added (an
    # owner of a cut tile); epilogue: the tiles this block stores
    return {"bid": bid, "segments": [], "deposit": None, "consumes": [], "epilogue": [], "idle": False, "lead": False}


def sk_ranges(total, G):
    """sk_start of every range 0 .. G: ranges of total // G or one more step, the longer ones first."""
    per, rem = divmod(total, G)
    return [r * per + min(r, rem) for r in range(G + 1)]


def _simulate_streamk(m_tiles, n_tiles, KT, reserved, compact=False):
    G = sk_workers(reserved)
    start = sk_ranges(m_tiles * n_tiles * KT, G)
    blocks = []
    for bid in range(G):
        b = _block(bid)
        r = (bid % NUM_XCD) * (G // NUM_XCD) + bid // NUM_XCD
        b["range"] = r
        it, it_end = start[r], start[r + 1]
        b["runs"] = []
        while True:                                           # (a do-while in the kernel: an empty range would still run once)
            tile = it // KT
            ks = it - tile * KT
            if compact and ks == 0 and it_end - it >= KT:
                # the whole tiles in the middle of a range as ONE entry (first tile, count): each is computed from K-step 0 to KT and
                # stored by this block, nothing is deposited or consumed -- what the loop below would say tile by tile
                count = (it_end - it) // KT
                b["runs"].append((tile, count))
                it += count * KT
                if not it < it_end:
                    break
                continue
            ke = min(KT, ks + (it_end - it))
            it += ke - ks
            b["segments"].append((tile, ks, ke))
            if ks > 0:
                b["deposit"] = r
            else:
                if ke < KT:
                    n = 1
                    while start[r + n + 1] < (tile + 1) * KT:      # (ends at range G at the latest: start[G] is the whole space)
                        n += 1
                    b["consumes"] += list(range(r + 1, r + n + 1))
                b["epilogue"].append(tile)
            if not it < it_end:
                break
        blocks.append(b)
    return {"kind": "stream-K", "blocks": blocks, "grid": G, "capacity": SK_SLOTS, "extent": SK_SLOTS * SLOT_BYTES,
            "m_tiles": m_tiles, "n_tiles": n_tiles, "KT": KT, "sk_per": start[G] // G, "sk_rem": start[G] % G}


def lead_tile(bid, m_tiles, n_tiles):
    """One block per tile: each XCD owns a contiguous run of pixel tiles.  The tile of block `bid`, None for a block without one."""
    per_xcd = ceil_div(n_tiles, NUM_XCD)
    xcd, slot = bid % NUM_XCD, bid // NUM_XCD
    n_local = slot // m_tiles
    n_tile = xcd * per_xcd + n_local
    if n_local >= per_xcd or n_tile >= n_tiles:
        return None
    return n_tile * m_tiles + slot % m_tiles


def lead_grid(m_tiles, n_tiles):
    return round_up_xcd(n_tiles) * m_tiles


def _lead_block(b, m_tiles, n_tiles, KT):
    tile = lead_tile(b["bid"], m_tiles, n_tiles)
    b["lead"] = True
    if tile is None:
        b["idle"] = True
        return
    b["segments"].append((tile, 0, KT))
    b["epilogue"].append(tile)


def _simulate_tiles(m_tiles, n_tiles, KT):
    grid = round_up_xcd(n_tiles) * m_tiles
    blocks = [_block(bid) for bid in range(grid)]
    for b in blocks:
        _lead_block(b, m_tiles, n_tiles, KT)
    return {"kind": "tile-per-block", "blocks": blocks, "grid": grid, "capacity": 0, "extent": 0, "m_tiles": m_tiles,
            "n_tiles": n_tiles, "KT": KT}


def tail_piece(q, xcd, R, split):
    """Piece q of the tail -> (tail tile, K-range index), None when the piece has no tile.  Later K-ranges come first."""
    per_x = ceil_div(R, NUM_XCD)
    part_rev = q // (per_x * NUM_XCD)
    ql = q - part_rev * (per_x * NUM_XCD)
    tr = xcd * per_x + ql // NUM_XCD
    if tr >= R:
        return None
    return tr, split - 1 - part_rev


def _simulate_tail(m_tiles, n_tiles, KT, split, lead_n, compact=False):
    R = (n_tiles - lead_n) * m_tiles
    lead_blocks = ceil_div(lead_n, NUM_XCD) * NUM_XCD * m_tiles
    grid = round_up_xcd(lead_n) * m_tiles + round_up_xcd(R) * split
    blocks = []
    for bid in range(lead_blocks if compact else 0, grid):   # (compact: the tail pieces only; the leading part is lead_tile's map)
        b = _block(bid)
        blocks.append(b)
        if bid < lead_blocks:
            _lead_block(b, m_tiles, lead_n, KT)
            continue
        piece = tail_piece(bid - lead_blocks, bid % NUM_XCD, R, split)
        if piece is None:
            b["idle"] = True
            continue
        tr, part = piece
        tile0 = lead_n * m_tiles + tr
        it = tile0 * KT + part * KT // split
        it_end = tile0 * KT + (part + 1) * KT // split
        tile = it // KT
        ks = it - tile * KT
        ke = min(KT, ks + (it_end - it))
        b["segments"].append((tile, ks, ke))
        b["piece"] = (tr, part)
        if ks > 0:
            b["deposit"] = tr * (split - 1) + part - 1
        else:
            if ke < KT:
                first = (tile - lead_n * m_tiles) * (split - 1)
                b["consumes"] += list(range(first, first + split - 1))
            b["epilogue"].append(tile)
    return {"kind": "tile+tail", "blocks": blocks, "grid": grid, "capacity": TAIL_SLOTS, "extent": TAIL_SLOTS * SLOT_BYTES,
            "m_tiles": m_tiles, "n_tiles": n_tiles, "KT": KT, "split": split, "lead_n": lead_n, "R": R, "lead_blocks": lead_blocks}


def simulate_gemm(m_tiles, n_tiles, KT, reserved, schedule, compact=False):
    """Every block of dasac_conv_gemm over a whole tensor of m_tiles x n_tiles 128 x 128 tiles and KT K-steps, given a workspace.
    schedule 0 = the library's choice (a split-K tail when tail_plan finds one, else stream-K when want_streamk, else one block
    per tile), 1 = one block per tile, 2 = stream-K (which falls back to one block per tile when the space has fewer steps than
    workers).  Returns the plan: kind, grid, the blocks with their segments / deposit slot / consumed slots / epilogue tiles.
    compact (for sweeps over large grids): a stream-K block lists the whole tiles in the middle of its range as `runs` of (first tile,
    count) instead of one segment each, and a tail plan holds its tail pieces only (blocks lead_blocks .. grid - 1); the leading part
    of a tail launch is the one-block-per-tile map of lead_n pixel tiles, lead_tile."""
    reserved = clamp_reserved(reserved)
    if schedule == 0:
        split, lead_n = tail_plan(m_tiles, n_tiles, KT, reserved)
        if split > 0:
            return _simulate_tail(m_tiles, n_tiles, KT, split, lead_n, compact)
    sk_ok = m_tiles * n_tiles * KT >= sk_workers(reserved)
    if sk_ok and (schedule == 2 or (schedule == 0 and want_streamk(m_tiles * n_tiles, KT, reserved))):
        return _simulate_streamk(m_tiles, n_tiles, KT, reserved, compact)
    return _simulate_tiles(m_tiles, n_tiles, KT)


# ----------------------------------------------------------------------------------------------
# device maps: the weight gradient
# ----------------------------------------------------------------------------------------------
def wgrad_ranges(Npix, splits, per):
    """[p_begin, p_end) of every split as the kernel computes them: p_end < = p_begin marks a split with no pixels."""
    return [(s * per, min(s * per + per, Npix)) for s in range(splits)]


def simulate_wgrad(M, K, Cx, Npix):
    """Every block of a dasac_conv_wgrad launch: (m_tile, k_tile, split, p_begin, p_end), None for a block past the list."""
    Mpad, Kpad, bm, bnk, splits = wgrad_layout(M, K, Cx, Npix)
    m_tiles, k_tiles = Mpad // bm, Kpad // bnk
    per = wgrad_per(Npix, splits)
    n_blocks = m_tiles * k_tiles * splits
    grid = round_up_xcd(n_blocks)
    per_xcd = ceil_div(n_blocks, NUM_XCD)
    blocks = []
    for bid in range(grid):
        lb = (bid % NUM_XCD) * per_xcd + bid // NUM_XCD
        if lb >= n_blocks:
            blocks.append(None)
            continue
        tile, split = lb % (m_tiles * k_tiles), lb // (m_tiles * k_tiles)
        p_begin = split * per
        blocks.append((tile % m_tiles, tile // m_tiles, split, p_begin, min(p_begin + per, Npix)))
    ranges = wgrad_ranges(Npix, splits, per)
    return {"kind": "wgrad", "blocks": blocks, "grid": grid, "Mpad": Mpad, "Kpad": Kpad, "bm": bm, "bnk": bnk, "m_tiles": m_tiles,
            "k_tiles": k_tiles, "splits": splits, "per": per, "Npix": Npix, "ranges": ranges,
            "empty": sum(1 for b, e in ranges if e <= b)}


# ----------------------------------------------------------------------------------------------
# what a plan exercises
# ----------------------------------------------------------------------------------------------
GEMM_FEATURES = ("range_inside_one_tile", "owner_only", "deposit_then_own", "deposit_then_whole_tiles", "whole_tiles_only",
                 "sk_rem_zero", "contributors >= 2", "contributors >= 64", "ragged_last_pixel_tile", "m_tiles > 1")
TAIL_FEATURES = ("tail_kt_not_divisible", "tail_pieces_return_early", "tail_lead_not_whole_round", "tail_split_below_8",
                 "tail_two_leading_rounds")
WGRAD_FEATURES = ("wgrad_empty_splits", "wgrad_last_split_partial_step", "wgrad_64_splits", "wgrad_cap_branch")
ALL_FEATURES = GEMM_FEATURES + TAIL_FEATURES + WGRAD_FEATURES


def features(plan, Npix=None):
    """Names of what a simulated plan exercises (`Npix`: the GEMM's pixel count, for the ragged last tile)."""
    f = set()
    if plan["kind"] == "wgrad":
        ranges = [(b, e) for b, e in plan["ranges"] if e > b]
        if plan["empty"]:
            f.add("wgrad_empty_splits")
        if (ranges[-1][1] - ranges[-1][0]) % WG_PIX:
            f.add("wgrad_last_split_partial_step")
        if plan["splits"] == 64:
            f.add("wgrad_64_splits")
        if plan["m_tiles"] * plan["k_tiles"] < 12 and plan["Npix"] >= 200000:
            f.add("wgrad_cap_branch")
        return f
    KT = plan["KT"]
    if plan["m_tiles"] > 1:
        f.add("m_tiles > 1")
    if Npix is not None and Npix % TILE:
        f.add("ragged_last_pixel_tile")
    whole = lambda s: s[1] == 0 and s[2] == KT
    if plan["kind"] == "stream-K":
        if plan["sk_rem"] == 0:
            f.add("sk_rem_zero")
        for b in plan["blocks"]:
            seg = b["segments"]
            if len(seg) == 1 and not whole(seg[0]):
                f.add("range_inside_one_tile")
                if seg[0][1] == 0:
                    f.add("owner_only")
            if all(whole(s) for s in seg):
                f.add("whole_tiles_only")
            if len(seg) > 1 and seg[0][1] > 0:
                if whole(seg[1]):
                    f.add("deposit_then_whole_tiles")
                if seg[-1][1] == 0 and seg[-1][2] < KT:
                    f.add("deposit_then_own")
            if len(b["consumes"]) >= 2:
                f.add("contributors >= 2")
            if len(b["consumes"]) >= 64:
                f.add("contributors >= 64")
    if plan["kind"] == "tile+tail":
        split = plan["split"]
        if KT % split:
            f.add("tail_kt_not_divisible")
        if plan["R"] % NUM_XCD:
            f.add("tail_pieces_return_early")
        if (plan["lead_n"] * plan["m_tiles"]) % TILE_SLOTS:
            f.add("tail_lead_not_whole_round")
        if 2 <= split < MAX_SPLIT:
            f.add("tail_split_below_8")
        if plan["lead_n"] * plan["m_tiles"] >= 2 * TILE_SLOTS:
            f.add("tail_two_leading_rounds")
        if split >= 3:
            f.add("contributors >= 2")
    return f
