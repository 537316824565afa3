"""The launch plans and block maps of the conv GEMM and the weight gradient (csrc/conv_plan.hpp: what the launchers and the kernels
themselves call) on the host: tools/conv_plan_check.cpp, a stand-alone program built with AddressSanitizer and UBSan (host code
only, its own `main`; no GPU, nothing loaded into Python), answers the requests this test writes to its stdin, and every answer is
compared with the independent restatement, gemm_schedule_ref.py.

Rules: the grid of test_gpu_gemm_schedule_rules.shapes() x reserved CUs {0, 8, 16, 64, 128} x full_chip {1, 0} -- schedule kind,
split, lead_n, grid and workspace of the GEMM; tiles, splits, pixels per split, grid, Psum offset and workspace of the weight
gradient (at both k-tile widths); the batched splits of the Winograd point shapes of tools/winograd_bits.py.  Without the full
chip every plan is one block per tile, and the label rule of ops.conv_gemm (whole tensor, workspace, schedule 0) is the plan's
kind: tail exactly when the tail-split query is positive, else stream-K exactly when the schedule query is 1.

Walks, through the header's own device maps: the one-block-per-tile GEMM map, which every SK = 0 instantiation of conv_gemm calls,
over the whole n_tiles spread of test_gemm_schedule_cpu.py for m_tiles 1 .. 9 and over the lead_n of every tail plan of its grid
(every tile reached once, by a block whose range is that whole tile; the tail kernel decodes its leading blocks with lines of its
own, so for it this checks the arithmetic, not its code); the weight-gradient map over WGRAD_CASES of conv_lattice (every block
printed and compared entry for entry with the model's walk) and over the batched shapes.  The program counts every broken promise
(see its head comment).  The stream-K and tail maps are written inside conv_gemm (moved to the header, one timing row of each
schedule missed its bound: profiles/conv_plan.md), so the walks of STREAMK_CASES, SCHEDULE_CASE, TAIL_CASE and TAIL_CASES have no
C++ function to run on: for those maps the model, checked against itself in test_gemm_schedule_cpu.py, remains the only check."""
import os
import subprocess
import sys

import pytest

import conv_lattice as cl
import gemm_schedule_ref as R
import test_gemm_schedule_cpu as G
from test_gpu_gemm_schedule_rules import shapes
from test_winograd_index_host import ROOT, _compiler

RESERVED = (0, 8, 16, 64, 128)


def _gemm_want(M, K, Npix, reserved, full):
    """(kind, grid, m_tiles, n_tiles, lead_n, tail_tiles, split, wants_streamk, uses_workspace, workspace_bytes) by the model."""
    bm = R.pick_bm(R.conv_mpad(M))
    bn = 256 if bm == 32 else 128
    m_tiles, n_tiles, KT = R.ceil_div(M, bm), R.ceil_div(Npix, bn), R.ceil_div(K, R.BK)
    wants = bool(full and bm == 128 and R.want_streamk(m_tiles * n_tiles, KT, reserved))
    split, lead_n = R.tail_plan(m_tiles, n_tiles, KT, reserved) if (full and bm == 128) else (0, 0)
    if split > 0:
        tail = (n_tiles - lead_n) * m_tiles
        return (2, R.round_up_xcd(lead_n) * m_tiles + R.round_up_xcd(tail) * split, m_tiles, n_tiles, lead_n, tail, split, 1, 1, R.gemm_workspace())
    if wants:
        return (1, R.sk_workers(reserved), m_tiles, n_tiles, 0, 0, 0, 1, 1, R.gemm_workspace())
    return (0, R.round_up_xcd(n_tiles) * m_tiles, m_tiles, n_tiles, 0, 0, 0, 0, 0, 0)


def _wgrad_want(M, K, Cx, Npix):
    Mpad, Kpad, bm, bnk, splits = R.wgrad_layout(M, K, Cx, Npix)
    m_tiles, k_tiles = Mpad // bm, Kpad // bnk
    return (Mpad, Kpad, bm, bnk, m_tiles, k_tiles, splits, R.wgrad_per(Npix, splits), R.round_up_xcd(m_tiles * k_tiles * splits),
            splits * Mpad * Kpad, R.wgrad_workspace(1, 1, Npix, M, K))


def _batched_want(batch, M, C, T):
    if M % 128 or C % 128 or T % 4:
        return (0, 0, 0, 0, 0)
    tiles = batch * (M // 128) * (C // 128)
    splits = R.fill_rounds(tiles, min(R.ceil_div(T, R.MIN_PIX), 64), R.WG_SLOTS)
    return (splits, R.wgrad_per(T, splits), R.round_up_xcd((M // 128) * (C // 128) * splits), splits * batch * M * C,
            splits * (batch * M * C + M) * 4)


def _tile_walks():
    """Requests and expected (kind, grid, m_tiles, n_tiles, KT, blocks with work) of the one-block-per-tile launches."""
    out = []
    for m_tiles in range(1, 10):
        ns = set(G.n_tiles_list(m_tiles))
        ns |= {R.tail_plan(m_tiles, n, KT, res)[1] for n in G.n_tiles_list(m_tiles) for KT in G.KTS for res in G.RESERVED
               if R.tail_plan(m_tiles, n, KT, res)[0]}
        for n in sorted(ns):                                                                  # (the map does not depend on KT)
            out.append(("walk {} {} {} 1 0".format(128 * m_tiles, 80, 128 * n), (0, R.lead_grid(m_tiles, n), m_tiles, n, 5, m_tiles * n)))
    return out


def _case_walks():
    """Requests, answer heads and the model's full walks of the weight-gradient kernel cases of conv_lattice."""
    out = []
    for case in cl.WGRAD_CASES:
        M, Npix, K = cl.gemm_shape(case)
        plan = R.simulate_wgrad(M, K, case[1], Npix)
        head = (plan["grid"], plan["m_tiles"], plan["k_tiles"], plan["splits"], plan["per"])
        out.append(("wwalk {} {} {} {} 1".format(M, K, case[1], Npix), head, [(-1,) * 5 if b is None else b for b in plan["blocks"]]))
    return out


@pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")
def test_conv_plans_equal_the_model_and_every_block_walk_keeps_its_promises(tmp_path):
    exe = tmp_path / "conv_plan_check"
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "da-sac_amd", "csrc"), os.path.join(ROOT, "tools", "conv_plan_check.cpp"), "-o", str(exe)])
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import winograd_bits
    finally:
        sys.path.pop(0)
    grid = shapes()
    assert len(grid) > 5000
    requests, checks = [], []                       # one check per answered line: (tag, payload)
    for Nb, OH, OW, M, K in grid:
        Npix = Nb * OH * OW
        for res in RESERVED:
            for full in (1, 0):
                requests.append("gemm {} {} {} 0 {} 0 1 {} {}".format(M, K, Npix, Npix, res, full))
                checks.append(("gemm", (M, K, Npix, res, full)))
        for Cx in (K, 64):                          # the 128-row k tile, and the 64-row one where the layout allows it
            requests.append("wgrad {} {} {} {}".format(M, K, Cx, Npix))
            checks.append(("wgrad", (M, K, Cx, Npix)))
    batched = [(P, 128, 128, T, want) for P, _ in winograd_bits.FORMS.values() for T, want in winograd_bits.FINISH_T]
    batched += [(16, 128, 128, 162, 0), (36, 128, 128, 100, 1)]        # F(2x2) at two samples: no multiple of 4, refused; F(4x4): taken
    for P, M, C, T, want in batched:
        requests.append("batched {} {} {} {}".format(P, M, C, T))
        checks.append(("batched", (P, M, C, T, want)))
    walks = _tile_walks()
    for req, want in walks:
        requests.append(req)
        checks.append(("walk", want))
    cases = _case_walks()
    for req, head, blocks in cases:
        requests.append(req)
        checks.append(("case", (head, blocks)))

    out = subprocess.run([str(exe)], input="\n".join(requests) + "\n", capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    lines = iter(out.stdout.splitlines())
    ints = lambda line, tag: tuple(int(v) for v in line.split()[1:]) if line.split()[0] == tag else pytest.fail(line)
    counts = {}
    for (tag, want), req in zip(checks, requests):
        line = next(lines)
        if tag == "gemm":
            M, K, Npix, res, full = want
            got = ints(line, "gemm")
            assert got == _gemm_want(M, K, Npix, res, full), (req, line)
            kind, split, wants = got[0], got[6], got[7]
            if not full:
                assert kind == 0, (req, line)                               # without the whole chip: one block per tile, always
            else:
                # the three queries and the label rule of ops.conv_gemm: the split-K tail goes first, then stream-K
                assert (split, wants) == (R.gemm_tail_split(1, 1, Npix, M, K, res), R.gemm_schedule(1, 1, Npix, M, K, res)), (req, line)
                assert (kind == 2) == (split > 0) and (split > 0 or (kind == 1) == (wants == 1)), (req, line)
                for name, hit in (("stream-K", wants), ("tail", split > 0), ("split<8", 0 < split < 8)):
                    counts[(res, name)] = counts.get((res, name), 0) + int(hit)
        elif tag == "wgrad":
            assert ints(line, "wgrad") == _wgrad_want(*want), (req, line)
        elif tag == "batched":
            got = ints(line, "batched")
            assert got == _batched_want(*want[:4]) and got[0] == want[4], (req, line)
        elif tag == "walk":
            assert ints(line, "walk") == want + (0,), (req, line)               # ... and 0 broken promises
        else:
            head, blocks = want
            assert line.split()[-1] == "-" and tuple(int(v) for v in line.split()[1:-1]) == head, (req, line)
            for bid, block in enumerate(blocks):
                assert tuple(int(v) for v in next(lines).split()[1:]) == (bid,) + tuple(block), (req, bid, block)
    last = next(lines)
    assert next(lines, None) is None
    print(last, "; reached per (reserved, answer):", counts)
    assert all(counts.get((res, name), 0) > 20 for res in RESERVED for name in ("stream-K", "tail", "split<8")), counts
    n_shapes = len(grid) * (len(RESERVED) * 2 + 2) + len(batched)
    n_plans = len(walks) + len(cases) + sum(1 for b in batched if b[4] > 0)
    assert last.startswith("conv plan check: {} shapes, {} plans walked, ".format(n_shapes, n_plans)) and last.endswith(" 0 bad"), last
    assert last == PINNED, last


PINNED = "conv plan check: 95322 shapes, 1168 plans walked, 13508648 blocks walked, 0 bad"
