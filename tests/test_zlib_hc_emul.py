"""CPU check of the high-compression zlib parse (tyche_amd/csrc/zlib_hc_core.h, pass 1 of
zlib_deflate_hc_kernel, ZLIB_HC=1) through its host emulator tools/zlib_hc_emul.cpp: the records of
every page tile it with true matches of at least 3 bytes inside deflate's window, the gains and the
lazy rule are the ones the header words, the cost rule refuses what it says it refuses, and the
records, costed with an exact dynamic-Huffman size, close half of the gap between the reference's
levels 1 and 6.  That size is an estimate of the device's stream (optimal length-limited codes); the
GPU tests (test_gpu_zlib_hc.py) hold the kernel's streams to the emulator's records and the mode to
its ratio on the device's own bytes."""
import ctypes
import json
import zlib as pyzlib

import numpy as np
import pytest

import zlib_hc_cases as C


@pytest.fixture(scope="module")
def emul():
    return C.load_emul()


@pytest.fixture(scope="module")
def cases(oracle_mod):
    return C.cpu_case_pages(oracle_mod)


def parsed(emul, page: bytes):
    recs, last = emul(page)
    C.check_records(recs, last, page)
    return recs, last


def xbits(d):
    return 0 if d <= 4 else (d - 1).bit_length() - 2


def test_records_tile_every_page_with_true_matches(emul, cases):
    lay = emul.layout
    for name, page in cases:
        recs, last = parsed(emul, page)
        for ls, ll, ml, d in recs:
            # the cost rule's bounds (a backward extension only makes a match longer)
            assert not (ml == 3 and d > lay["far3"]), (name, ls, ll, ml, d)
            assert not (ml == 4 and d > lay["far4"]), (name, ls, ll, ml, d)
        if len(page) < 4:
            assert recs == [] and last == len(page), name
        assert sum(C.chunks(ml) != [] and sum(C.chunks(ml)) == ml and min(C.chunks(ml)) >= 3 and max(C.chunks(ml)) <= 258
                   for _, _, ml, _ in recs) == len(recs), name
    assert emul(b"") == ([], 0)


def test_gains_and_the_lazy_rule_are_the_headers(emul, cases):
    """The emulator's trace gives every block's base, the cursor it started from, the lanes whose
    match stands and each lane's (gain, length, candidate).  Restated here: the gain formula and
    its two refusals, the standing lanes from the neighbours' gains, and the walk -- the first
    standing lane at or after the cursor, extended backwards by at most back_max bytes and never
    below the cursor, its end the new cursor -- which must give the records one for one."""
    lay = emul.layout
    W, G0, S, P = lay["len_w"], lay["gain_base"], lay["stride"], lay["probe"]
    for name, page in cases:
        if len(page) > 20000 and not name.startswith("distance"):
            continue
        a = np.frombuffer(page, np.uint8)
        recs, last = emul(page)
        i = 0
        n = len(page)
        for blk in emul.trace(page):
            base, cursor = int(blk[0]), int(blk[1])
            E = int(blk[2]) | (int(blk[3]) << 32)
            gn, ln, cd = blk[4::3].tolist(), blk[5::3].tolist(), blk[6::3].tolist()
            for k in range(64):
                q = base + k
                if gn[k] == 0:
                    continue
                d = q - cd[k]
                assert q <= n - 3 and 3 <= ln[k] <= P and 1 <= d <= C.MAX_DIST and q + ln[k] <= n, (name, q)
                assert np.array_equal(a[q:q + ln[k]], a[cd[k]:cd[k] + ln[k]]), (name, q)
                assert not (ln[k] == 3 and d > lay["far3"]) and not (ln[k] == 4 and d > lay["far4"]), (name, q, d)
                assert gn[k] == W * ln[k] + G0 - xbits(d), (name, q, gn[k], ln[k], d)
            want = 0
            for k in range(S):
                g0, g1, g2 = gn[k], gn[k + 1], gn[k + 2]
                if g0 and not (g1 > g0 + lay["lazy1"] or g2 > g0 + lay["lazy2"]):
                    want |= 1 << k
            assert E == want, (name, base, hex(E), hex(want))
            s = max(cursor - base, 0)
            while s < S and E >> s:
                s += ((E >> s) & -(E >> s)).bit_length() - 1
                pos = base + s
                ls, ll, ml, d = recs[i]
                end = ls + ll + ml
                assert ls == cursor and ls + ll <= pos < end and pos - (ls + ll) <= lay["back_max"], (name, pos, recs[i])
                assert d == pos - cd[s], (name, pos, recs[i])
                full = end - pos
                assert full == ln[s] if ln[s] < P else full >= P, (name, pos, full, ln[s])
                back = pos - (ls + ll)
                # the backward extension stops at the cursor, at the candidate's position 0, at its limit or at a differing byte
                assert back == min(pos - cursor, cd[s], lay["back_max"]) or a[pos - back - 1] != a[pos - d - back - 1], (name, pos)
                # and the full length stops at the page's end or at a differing byte
                assert end == n or a[end] != a[end - d], (name, pos, end)
                i += 1
                cursor = end
                s = cursor - base
        assert i == len(recs), (name, i, len(recs))


def test_shapes_the_parse_must_get_right(emul, cases):
    by = dict(cases)
    for m in C.EXACT_LENS:
        recs, _ = parsed(emul, by[f"exact/{m}"])
        assert (m, m + 300) in [(ml, d) for _, _, ml, d in recs], (m, recs)
    recs, _ = parsed(emul, by["distance/32768"])
    assert any(d == 32768 and ml >= 40 for _, _, ml, d in recs), recs[-3:]
    recs, _ = parsed(emul, by["distance/32769"])
    assert not any(ml >= 40 and d != 1 for _, _, ml, d in recs), [r for r in recs if r[2] >= 40]   # (d 1: the zero run)
    recs, _ = parsed(emul, by[f"three/{C.NEAR3}"])
    assert (3, C.NEAR3) in [(ml, d) for _, _, ml, d in recs]
    recs, _ = parsed(emul, by[f"three/{C.FAR3}"])
    assert C.FAR3 > emul.layout["far3"] and not any(d == C.FAR3 for _, _, _, d in recs)
    for shift in (0, 5, 61):
        for kind, period in (("run", 1), ("period2", 2), ("period3", 3), ("period5", 5)):
            recs, last = parsed(emul, by[f"{kind}/{shift}"])
            n = 700 // period * period
            assert sum(ml for _, _, ml, d in recs if d == period) >= n - period - 2, (kind, shift, recs[:4])
    page, pos, dist = C.crowded_page()
    recs, _ = parsed(emul, page)
    assert emul.layout["ways"] < 62 and C.CROWDED_KEPT + 3 <= emul.layout["ways"]
    # the 30-byte repeat from the run's last 10 bytes on: found only if the ring kept the bucket's latest positions
    assert [(ls + ll, ml, d) for ls, ll, ml, d in recs if ls + ll == pos] == [(pos, C.CROWDED_KEPT + 20, dist)], recs[-4:]
    for n in (100, 4096):
        page = by[f"random/{n}"]
        recs, last = parsed(emul, page)
        assert C.stream_size(recs, last, page) == 2 + n + 5 + 4      # incompressible: the stored form


def test_walker_on_stored_fixed_and_dynamic_blocks(oracle_mod, cases):
    """The symbol walker on streams of other encoders: the bytes it decodes are the page and what the
    reference's uncompress gives, for stored (level 0), fixed (short pages) and dynamic blocks."""
    O = oracle_mod
    seen = set()
    for name, page in cases:
        if len(page) > 20000:
            continue
        streams = [pyzlib.compress(page, 0), pyzlib.compress(page, 6)]
        if O.have_ref():
            streams += [O.ref_zlib_compress(page, 1), O.ref_zlib_compress(page, 6)]
        for s in streams:
            syms, dec, kinds = C.walk(s)
            seen.update(kinds)
            assert dec == page, name
            assert sum(1 if isinstance(x, int) else x[0] for x in syms) == len(page)
            if O.have_ref():
                assert O.ref_zlib_uncompress(s, len(page)) == (len(page), page), name
    assert seen == {0, 1, 2}


def test_emulator_closes_half_of_the_gap_to_level_6(emul, oracle_mod):
    """Totals over 48 pagegen pages per cell (tests/golden/zlib_hc_targets.json): the emulator's
    records at their exact dynamic-Huffman size against the reference's compress2 at levels 1 and 6.
    At least half of the gap in each of the nine cells of distributions 0, 1 and 5."""
    t = C.targets()["cells"]
    failures = []
    for dist in C.RATIO_DISTS:
        for plen in C.RATIO_LENS:
            l1, l6 = t[f"{dist}/{plen}"]
            total = 0
            for p in C.ratio_pages(oracle_mod, dist, plen):
                page = p.tobytes()
                recs, last = emul(page)
                total += C.stream_size(recs, last, page)
            share = (l1 - total) / (l1 - l6)
            print(json.dumps({"dist": dist, "page_len": plen, "emulator": total, "level1": l1, "level6": l6,
                              "share_closed": round(share, 3)}))
            if total > C.ratio_bar(l1, l6):
                failures.append((dist, plen, l1, l6, total, round(share, 3)))
    assert not failures, failures


def test_targets_are_the_reference_librarys(oracle_mod):
    """Where oracle/_ref is built, the recorded totals are what its compress2 gives now."""
    O = oracle_mod
    if not O.have_ref():
        pytest.skip("oracle/_ref is not built")
    t = C.targets()["cells"]
    assert set(t) == {f"{d}/{n}" for d in C.RATIO_DISTS + C.NOGROW_DISTS for n in C.RATIO_LENS}
    for key in ("0/4096", "1/16384", "5/32768", "2/4096"):
        dist, plen = (int(x) for x in key.split("/"))
        pages = C.ratio_pages(O, dist, plen)
        assert [sum(len(O.ref_zlib_compress(p.tobytes(), lv)) for p in pages) for lv in (1, 6)] == t[key], key


def test_out_of_range_arguments(emul):
    buf = (ctypes.c_uint8 * 16)()
    recs = (ctypes.c_uint32 * 64)()
    last = ctypes.c_uint32(0)
    assert emul.lib.zlibhc_emul_parse(buf, 65536, recs, 16, ctypes.byref(last)) == -2 ** 31
    assert emul.lib.zlibhc_emul_parse(buf, -1, recs, 16, ctypes.byref(last)) == -2 ** 31
