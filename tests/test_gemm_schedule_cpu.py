"""Properties of the conv GEMM's hand-off schedules and of the weight gradient's pixel splits, checked on the model of
gemm_schedule_ref.py without a GPU: every (tile, K-step) is computed exactly once, every tile has one owner, every deposit slot
is written once, read once by that owner and lies inside its buffer, no range or piece is empty, the tail cannot wait on a block
that is dispatched later, and the weight gradient's splits tile the pixel axis inside the workspace it states.  Then: the case
lists of test_gpu_conv_schedules_exact.py reach every feature the model names -- a condition on the inputs, checked here before any
kernel runs.  (test_gpu_gemm_schedule_rules.py holds the model's host half against the shipped library.)"""
import pytest

import conv_lattice as cl
import gemm_schedule_ref as R

KTS = (1, 8, 15, 16, 63, 64, 65, 72, 73, 144, 288, 2048)
RESERVED = cl.RESERVED                  # reserved CUs: (0, 8, 64, 128)
SPREAD = (1, 2, 3, 5, 8, 9, 17, 31, 64, 100, 129, 255, 296, 500, 768, 1000, 1178, 1500, 2000, 2500, 3000, 3500, 4000)


def n_tiles_list(m_tiles):
    """A spread from 1 to 4000 with every value within 2 of a multiple of 1024 / m_tiles (both roundings of a fractional one)."""
    vals = set(SPREAD)
    k = 1
    while k * R.TILE_SLOTS // m_tiles - 2 <= 4000:
        for base in (k * R.TILE_SLOTS // m_tiles, R.ceil_div(k * R.TILE_SLOTS, m_tiles)):
            vals.update(range(base - 2, base + 3))
        k += 1
    return sorted(v for v in vals if 1 <= v <= 4000)


def check_plan(plan):
    """Coverage, ownership, slots and progress of one simulated launch (compact or not; of a compact tail plan: its tail part)."""
    KT, m_tiles, tiles = plan["KT"], plan["m_tiles"], plan["m_tiles"] * plan["n_tiles"]
    what = (plan["kind"], m_tiles, plan["n_tiles"], KT, plan["grid"], plan.get("split"), plan.get("lead_n"))
    assert 0 < plan["grid"] < 2 ** 31, what
    tile_lo = 0
    if plan["kind"] == "tile+tail" and plan["blocks"][0]["bid"] > 0:
        tile_lo = plan["lead_n"] * m_tiles                  # the leading tiles belong to blocks this plan does not hold
        assert plan["blocks"][0]["bid"] == plan["lead_blocks"] == R.lead_grid(m_tiles, plan["lead_n"]), what
    assert plan["blocks"][-1]["bid"] == plan["grid"] - 1, what
    parts = {}                 # cut tile -> [(ks, ke)]
    spans = []                 # (first tile, one past the last) of every run of whole tiles
    depositor = {}             # slot -> (bid, tile)
    for b in plan["blocks"]:
        runs = b.get("runs", ())
        assert b["idle"] == (not b["segments"] and not runs), what
        for tile, ks, ke in b["segments"]:
            assert 0 <= ks < ke <= KT and tile_lo <= tile < tiles, (what, b)    # no empty range, no empty piece
            if ks == 0 and ke == KT:
                spans.append((tile, tile + 1))
            else:
                parts.setdefault(tile, []).append((ks, ke))
        for first, count in runs:
            assert count >= 1 and tile_lo <= first and first + count <= tiles, (what, b)
            spans.append((first, first + count))
        assert b["epilogue"] == [t for t, ks, ke in b["segments"] if ks == 0], (what, b)                 # the owner holds K-step 0
        if b["deposit"] is not None:
            slot = b["deposit"]
            assert slot not in depositor, (what, slot)                          # written at most once
            assert 0 <= slot < plan["capacity"], (what, slot)
            assert slot * R.SLOT_BYTES + R.SLOT_BYTES <= plan["extent"] < 2 ** 31, (what, slot)
            assert b["segments"][0][1] > 0 and all(s[1] == 0 for s in b["segments"][1:]), (what, b)   # a range deposits at its start only
            depositor[slot] = (b["bid"], b["segments"][0][0])
        if b["lead"]:
            assert not b["consumes"] and b["deposit"] is None, (what, b)        # no lead block waits
    for tile, iv in parts.items():             # a cut tile: its pieces tile [0, KT), so exactly one of them holds K-step 0
        iv.sort()
        assert iv[0][0] == 0 and iv[-1][1] == KT and all(a[1] == b[0] for a, b in zip(iv, iv[1:])), (what, tile, iv)
        spans.append((tile, tile + 1))
    spans.sort()                               # every tile exactly once: whole in one block or cut among several
    assert spans[0][0] == tile_lo and spans[-1][1] == tiles and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), what
    consumed = set()
    for b in plan["blocks"]:
        if not b["consumes"]:
            continue
        cut = [t for t, ks, ke in b["segments"] if ks == 0 and ke < KT]
        assert len(cut) == 1, (what, b)
        for slot in b["consumes"]:
            assert slot not in consumed, (what, slot)                           # consumed exactly once ...
            consumed.add(slot)
            assert slot in depositor and depositor[slot][1] == cut[0], (what, b, slot)   # ... by its tile's owner
            if plan["kind"] == "tile+tail":
                assert depositor[slot][0] < b["bid"], (what, b, slot)           # later K-ranges carry lower block ids
    assert consumed == set(depositor), what
    return len(depositor)


def check_lead_map(m_tiles, n_tiles):
    """One block per tile over n_tiles pixel tiles (a whole launch, or the leading part of a tail launch): every tile once."""
    got = [R.lead_tile(bid, m_tiles, n_tiles) for bid in range(R.lead_grid(m_tiles, n_tiles))]
    got = sorted(t for t in got if t is not None)
    assert got == list(range(m_tiles * n_tiles)), (m_tiles, n_tiles)


def check_chosen(m_tiles, n_tiles, KT, reserved):
    split, lead_n = R.tail_plan(m_tiles, n_tiles, KT, reserved)
    if split == 0:
        return 0
    Rt = (n_tiles - lead_n) * m_tiles
    assert 1 <= split <= 8 and split * 8 <= KT and 0 < lead_n < n_tiles and Rt * (split - 1) <= R.TAIL_SLOTS
    assert R.round_up_xcd(lead_n) * m_tiles + R.round_up_xcd(Rt) * split < 2 ** 31
    assert R.want_streamk(m_tiles * n_tiles, KT, reserved)
    return split


@pytest.mark.parametrize("m_tiles", range(1, 10))
def test_chosen_tail_plans_fit_their_slots_and_their_k_steps(m_tiles):
    plans = sum(1 for n in n_tiles_list(m_tiles) for KT in KTS for res in RESERVED if check_chosen(m_tiles, n, KT, res))
    assert plans > 0


def test_reserved_cus_are_whole_cus_per_xcd_up_to_half_the_chip():
    for n in range(-3, 300):
        c = R.clamp_reserved(n)
        assert c % 8 == 0 and 0 <= c <= 128 and (c >= n or c == 128) and R.sk_workers(c) % 8 == 0 and R.sk_workers(c) <= R.SK_SLOTS
    assert [R.clamp_reserved(n) for n in (0, 1, 8, 13, 64, 127, 128, 129)] == [0, 8, 8, 16, 64, 128, 128, 128]


@pytest.mark.parametrize("m_tiles", range(1, 10))
def test_one_block_per_tile_reaches_every_tile_once(m_tiles):
    """The whole n_tiles spread, and the leading part of every tail plan of the grid (the map does not depend on KT)."""
    ns = set(n_tiles_list(m_tiles))
    ns |= {R.tail_plan(m_tiles, n, KT, res)[1] for n in n_tiles_list(m_tiles) for KT in KTS for res in RESERVED if R.tail_plan(m_tiles, n, KT, res)[0]}
    for n in sorted(ns):
        check_lead_map(m_tiles, n)
    check_plan(R.simulate_gemm(m_tiles, 1178, 5, 0, 1))                         # the block form of the same map


def test_every_tail_plan_of_the_grid_hands_off_through_its_own_slots():
    """EVERY tail plan of the whole grid (m_tiles 1 .. 9 x the n_tiles spread x 12 K lengths x 4 reserved settings) is walked piece
    by piece; plans that agree in (m_tiles, n_tiles, lead_n, split, KT) are the same launch and are walked once.  The leading
    blocks of these launches are checked in test_one_block_per_tile_reaches_every_tile_once."""
    splits, mid = {}, {}
    for m_tiles in range(1, 10):
        seen, per_x = set(), set()
        for n in n_tiles_list(m_tiles):
            for KT in KTS:
                for res in RESERVED:
                    split, lead_n = R.tail_plan(m_tiles, n, KT, res)
                    key = (lead_n, n, split, KT)
                    if split == 0 or key in seen:
                        continue
                    seen.add(key)
                    plan = R.simulate_gemm(m_tiles, n, KT, res, 0, compact=True)
                    assert plan["kind"] == "tile+tail" and (plan["split"], plan["lead_n"]) == (split, lead_n)
                    assert check_plan(plan) == plan["R"] * (split - 1)          # every non-owner piece deposits
                    splits[split] = splits.get(split, 0) + 1
                    per_x.add(R.ceil_div(plan["R"], 8))
                    if 16 <= plan["R"] <= 900 and split > 1:
                        mid[m_tiles] = mid.get(m_tiles, 0) + 1
        print("m_tiles = {}: {} distinct tail plans walked, tail tiles per XCD {} .. {}: {}".format(
            m_tiles, len(seen), min(per_x), max(per_x), sorted(per_x)))
        assert min(per_x) <= 2 and max(per_x) >= 100                             # few and many tail tiles per XCD
    print("tail plans walked per split:", sorted(splits.items()), "; with 16 .. 900 tail tiles and a hand-off, per m_tiles:", mid)
    # the walk reached the regime the tail exists for: every split from 1 to 8, and mid-range tails that hand off for every m_tiles
    assert all(splits.get(sp, 0) >= 3 for sp in range(1, 9)), splits
    assert all(mid.get(m, 0) >= 3 for m in range(1, 10)), mid


_CROSS = [(KT, res) for KT in KTS for res in RESERVED]


def _streamk_cross(i):
    """Two (KT, reserved) pairs for the i-th large grid, rotating through the whole cross of 48 every 24 grids."""
    return [_CROSS[(2 * i + j) % len(_CROSS)] for j in range(2)]


def test_every_stream_k_range_walk_covers_the_space_once():
    """Stream-K wherever it can run, on the WHOLE n_tiles spread of every m_tiles.  Grids up to a little past one round of 1024
    tiles take every K length with no reserved CUs and two lengths with 8, 64 and 128; every larger grid -- ranges that span many
    tiles -- takes two (K length, reserved) pairs that rotate through the whole cross from one grid to the next.  Thinned in K
    length and reserved CUs, never in n_tiles.  The map depends on the tile COUNT, the K length and the worker count alone, so a
    launch that another m_tiles already gave is not walked again."""
    seen, pairs = set(), set()
    for m_tiles in range(1, 10):
        walked = spanning = 0
        for i, n in enumerate(n_tiles_list(m_tiles)):
            tiles = m_tiles * n
            if tiles <= R.TILE_SLOTS + 3 * m_tiles:
                cross = [(KT, res) for KT in KTS for res in RESERVED if res == 0 or KT in (73, 288)]
            else:
                cross = _streamk_cross(i)
            for KT, res in cross:
                if tiles * KT < R.sk_workers(res):
                    continue                                                    # (falls back to one block per tile)
                pairs.add((KT, res))
                spanning += tiles >= 3 * R.sk_workers(res)                      # ranges of 3 or more tiles
                if (tiles, KT, res) in seen:
                    continue
                seen.add((tiles, KT, res))
                plan = R.simulate_gemm(m_tiles, n, KT, res, 2, compact=True)
                assert plan["kind"] == "stream-K" and plan["grid"] == R.sk_workers(res)
                check_plan(plan)
                walked += 1
        print("m_tiles = {}: {} new stream-K launches walked; {} of this m_tiles have ranges of 3 or more tiles".format(m_tiles, walked, spanning))
        assert spanning >= 4
    assert len(pairs) == len(_CROSS) and len(seen) > 2000


def test_the_compact_walk_is_the_block_by_block_walk():
    """`compact` only abbreviates: expanding its runs of whole tiles gives the segments of the plain walk, block for block."""
    for m_tiles, n, KT, res in ((8, 200, 16, 0), (2, 589, 288, 8), (3, 8, 73, 64), (1, 4000, 1, 128), (9, 117, 2048, 0)):
        full, short = R.simulate_gemm(m_tiles, n, KT, res, 2), R.simulate_gemm(m_tiles, n, KT, res, 2, compact=True)
        assert full["kind"] == short["kind"] == "stream-K"
        for a, b in zip(full["blocks"], short["blocks"]):
            whole = [(t, 0, KT) for first, count in b["runs"] for t in range(first, first + count)]
            assert sorted(a["segments"]) == sorted(b["segments"] + whole)
            assert (a["deposit"], a["consumes"]) == (b["deposit"], b["consumes"])
    for m_tiles, n, KT, res in ((8, 153, 73, 0), (3, 346, 65, 0), (5, 215, 65, 8)):
        full, short = R.simulate_gemm(m_tiles, n, KT, res, 0), R.simulate_gemm(m_tiles, n, KT, res, 0, compact=True)
        assert full["blocks"][full["lead_blocks"]:] == short["blocks"] and all(b["lead"] for b in full["blocks"][:full["lead_blocks"]])
        check_plan(full)


def test_a_range_that_spans_tiles_and_the_real_network_grid():
    """The step's own long-K launch (1178 tiles x 288 steps) and its reserved-CU variants: a range spans two or three tiles."""
    for res in (0, 8, 64, 128):
        plan = R.simulate_gemm(2, 589, 288, res, 2)
        assert plan["kind"] == "stream-K" and plan["grid"] == R.sk_workers(res)
        check_plan(plan)
        assert {"deposit_then_own", "deposit_then_whole_tiles"} <= R.features(plan)


# ----------------------------------------------------------------------------------------------
# weight gradient
# ----------------------------------------------------------------------------------------------
def _layouts():
    """(Mpad, Kpad, bm, bnk) of the weight-gradient cases (the split count depends on the tile count alone)."""
    out = []
    for c in cl.WGRAD_CASES:
        M, Npix, K = cl.gemm_shape(c)
        lay = R.wgrad_layout(M, K, c[1], Npix)[:4]
        if lay not in out:
            out.append(lay)
    return out


def test_wgrad_pixel_splits_tile_the_pixel_axis_inside_the_stated_workspace():
    npixs = list(range(1, 20001)) + list(range(200000 - 300, 200000 + 301)) + [1200000]
    layouts = _layouts()
    assert len({(Mp // bm) * (Kp // bnk) for Mp, Kp, bm, bnk in layouts}) >= 5
    most_empty = {}
    for Mpad, Kpad, bm, bnk in layouts:
        tiles = (Mpad // bm) * (Kpad // bnk)
        for Npix in npixs:
            splits = R.wgrad_splits(Mpad, Kpad, Npix, bm, bnk)
            per = R.wgrad_per(Npix, splits)
            assert 1 <= splits <= (768 if tiles < 12 and Npix >= 200000 else 64) and per % R.WG_PIX == 0 and splits * per >= Npix
            cover = empty = 0
            for s in range(splits):                                     # the ranges tile [0, Npix) exactly
                b, e = s * per, min(s * per + per, Npix)
                if e > b:
                    assert b == cover and empty == 0
                    cover = e
                else:
                    empty += 1
            assert cover == Npix
            # the stated size (the larger split count of both k-tile widths) holds the slabs and the channel sums of this launch
            stated = max(R.wgrad_splits(Mpad, Kpad, Npix, bm, w) for w in (128, 64)) * Mpad * (Kpad + 1) * 4
            assert stated >= splits * Mpad * (Kpad + 1) * 4 and stated < 2 ** 40
            assert R.round_up_xcd(tiles * splits) < 2 ** 31 and (splits - 1) * per + per < 2 ** 31
            if empty > most_empty.get(tiles, (0, 0))[0]:
                most_empty[tiles] = (empty, Npix, splits)
    print("most empty trailing splits per tile count (empty, Npix, splits):", most_empty)
    def first_empty(Mpad, Kpad):                                           # the fewest pixels with an empty trailing split
        def last_begin(n):
            s = R.wgrad_splits(Mpad, Kpad, n, 128)
            return (s - 1) * R.wgrad_per(n, s)
        return min(n for n in npixs if last_begin(n) >= n)
    # 12 splits of 288 over 3073 pixels on four tiles (13 splits allowed, 12 fill the rounds as well); one tile: 16 over 4097
    assert (first_empty(256, 256), first_empty(128, 128), first_empty(128, 1152)) == (3073, 4097, 2561)


@pytest.mark.parametrize("case", cl.WGRAD_CASES, ids=[c[0] for c in cl.WGRAD_CASES])
def test_wgrad_block_map_reaches_every_tile_of_every_split_once(case):
    M, Npix, K = cl.gemm_shape(case)
    plan = R.simulate_wgrad(M, K, case[1], Npix)
    live = [b for b in plan["blocks"] if b is not None]
    assert len(live) == plan["m_tiles"] * plan["k_tiles"] * plan["splits"] and len(plan["blocks"]) == plan["grid"] < len(live) + 8
    assert len({b[:3] for b in live}) == len(live)
    assert all(0 <= mt < plan["m_tiles"] and 0 <= kt < plan["k_tiles"] and (pb, pe) == plan["ranges"][s] for mt, kt, s, pb, pe in live)
    assert R.wgrad_workspace(1, 1, Npix, M, K) >= plan["splits"] * plan["Mpad"] * (plan["Kpad"] + 1) * 4
    print("{}: bm {} bnk {} tiles {} x {}, {} splits of {}, {} empty".format(case[0], plan["bm"], plan["bnk"], plan["m_tiles"],
                                                                            plan["k_tiles"], plan["splits"], plan["per"], plan["empty"]))


# ----------------------------------------------------------------------------------------------
# the case lists of test_gpu_conv_schedules_exact.py
# ----------------------------------------------------------------------------------------------
def case_plans():
    """name -> (plan, features) of every launch the exact kernel tests make."""
    out = {}
    for c in cl.STREAMK_CASES + [cl.SCHEDULE_CASE]:
        M, Npix, K = cl.gemm_shape(c)
        for res in (cl.RESERVED if c in cl.STREAMK_RESERVED_CASES else (0,)):
            plan = R.simulate_gemm(*R.gemm_tiles(1, 1, Npix, M, K), res, 2)
            out["stream-K/{}/r{}".format(c[0], res)] = (plan, R.features(plan, Npix))
    for c in cl.TAIL_CASES:
        M, Npix, K = cl.gemm_shape(c)
        plan = R.simulate_gemm(*R.gemm_tiles(1, 1, Npix, M, K), cl.TAIL_RESERVED.get(c[0], 0), 0)
        out["tail/" + c[0]] = (plan, R.features(plan, Npix))
    for c in cl.WGRAD_CASES:
        M, Npix, K = cl.gemm_shape(c)
        plan = R.simulate_wgrad(M, K, c[1], Npix)
        out["wgrad/" + c[0]] = (plan, R.features(plan))
    return out


def test_the_kernel_cases_reach_every_named_feature():
    plans = case_plans()
    for name, (plan, feats) in plans.items():
        kind = name.split("/")[0]
        assert plan["kind"] == {"stream-K": "stream-K", "tail": "tile+tail", "wgrad": "wgrad"}[kind], name
        if kind != "wgrad":
            check_plan(plan)
        print(name, sorted(feats))
    reached = set().union(*(f for _, f in plans.values()))
    assert reached == set(R.ALL_FEATURES), set(R.ALL_FEATURES) - reached
    # and the plans the cases were written for
    f = lambda n: plans[n][1]
    p = lambda n: plans[n][0]
    assert (p("stream-K/spans/r0")["sk_per"], p("stream-K/spans/r0")["sk_rem"]) == (33, 256)
    assert {"deposit_then_own", "deposit_then_whole_tiles"} <= f("stream-K/spans/r0")
    assert (p("stream-K/whole_tile_ranges/r0")["sk_per"], p("stream-K/whole_tile_ranges/r0")["sk_rem"]) == (16, 512)
    assert "whole_tiles_only" in f("stream-K/whole_tile_ranges/r0") and "sk_rem_zero" in f("stream-K/aligned/r0")
    assert max(len(b["consumes"]) for b in p("stream-K/many_contributors/r0")["blocks"]) == 143
    assert {"ragged_last_pixel_tile", "m_tiles > 1"} <= f("stream-K/ragged/r0") and p("stream-K/three_m_tiles/r0")["m_tiles"] == 3
    assert [p("stream-K/spans/r%d" % r)["grid"] for r in cl.RESERVED] == [768, 744, 576, 384]
    tail = {n: (p("tail/" + n)["split"], p("tail/" + n)["lead_n"], p("tail/" + n)["R"]) for n in [c[0] for c in cl.TAIL_CASES]}
    assert tail == {"split5": (5, 128, 200), "m3": (8, 341, 15), "m5": (8, 204, 55), "two_rounds": (8, 256, 32), "reserved8": (8, 128, 96)}
    assert {"tail_kt_not_divisible", "tail_split_below_8", "ragged_last_pixel_tile"} <= f("tail/split5")
    assert {"tail_pieces_return_early", "tail_lead_not_whole_round"} <= f("tail/m3") and "tail_two_leading_rounds" in f("tail/two_rounds")
    wg = {n: (p("wgrad/" + n)["splits"], p("wgrad/" + n)["per"], p("wgrad/" + n)["empty"]) for n in [c[0] for c in cl.WGRAD_CASES]}
    assert wg == {"quad": (16, 288, 1), "qtap": (16, 288, 1), "k_tile_64": (16, 288, 1), "strided_fast": (16, 352, 0), "generic": (20, 288, 1),
                  "bm64": (18, 320, 1), "splits64": (64, 288, 6), "splits64_3x3": (64, 288, 6), "cap_branch": (768, 288, 71), "cap_branch_stem": (384, 544, 13)}
    assert p("wgrad/k_tile_64")["bnk"] == 64 and p("wgrad/generic")["bm"] == 32 and p("wgrad/bm64")["bm"] == 64
