"""Selected match (include/hrx.h SELECTED) on host-only contexts: hrx_match_selected_host over a string-major and a ragged source gives every selected
string what hrx_match_batch_host / hrx_match_batch_host_ragged give it on the same batch (which tests/test_match_cpu.py and tests/test_ragged_cpu.py pin
to the oracle) and touches no other entry; selections in any order, with indices past the batch; tile-edge and bad lengths; argument checks; the
describe texts of the selected layouts, and those of the unselected layouts as they were before."""
import ctypes as C

import numpy as np
import pytest

import halo2_regex_amd as hra
from halo2_regex_amd import synth
from test_match_cpu import CFG_1, CFG_23, CFG_H3, CFG_H4, _cfg

BAD_LENGTH = 3
M = 208
MAX_SPANS = 8
P64, P32 = np.uint64(0xDEADBEEFCAFEF00D), np.uint32(0xABABABAB)
CFGS = [("regex1", CFG_1), ("regex23", CFG_23), ("headers3", CFG_H3), ("headers4", CFG_H4)]
SEL = hra.LAYOUT_INPUT_SELECTED if hasattr(hra, "LAYOUT_INPUT_SELECTED") else 16


def edge_batch(seed=5):
    """strings at the tile edges 0, 1, 15, 16, 17, 63, 64, 65, M - 1, M and M + 1 (bad length), three of each, shuffled: chars [B][stride], lens"""
    edge = [0, 1, 15, 16, 17, 63, 64, 65, M - 1, M, M + 1]
    rng = np.random.default_rng(seed)
    body, _ = synth.reveal_stress(len(edge) * 3, M + 1, seed=3)
    stride = -(-(M + 1) // 16) * 16
    lens = np.array(edge * 3, np.uint32)[rng.permutation(len(edge) * 3)]
    chars = np.zeros((len(lens), stride), np.uint8)
    chars[:, :body.shape[1]] = body[:, :stride]
    chars[np.arange(stride)[None, :] >= lens.astype(np.int64)[:, None]] = 0
    return chars, lens


def column(chars, lens, lead=3):
    """the same strings back to back after `lead` bytes, with one decreasing offset pair (string 7 has no valid length; string 8 then starts a byte early)"""
    L = lens.astype(np.int64)
    offsets = np.zeros(len(L) + 1, np.int64)
    np.cumsum(L, out=offsets[1:])
    offsets += lead
    values = np.full(-(-int(offsets[-1]) // 16) * 16 + 16, 0xAA, np.uint8)
    values[lead:int(offsets[-1])] = chars[np.arange(chars.shape[1])[None, :] < L[:, None]]
    offsets[8] = offsets[7] - 1
    return values, offsets.astype(np.uint64)


def selections(B, seed=1):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(B).astype(np.uint32)
    mixed = np.concatenate([perm[:B // 2], np.array([B, B + 7, 0xFFFFFFFF], np.uint32), perm[B // 2:B // 2 + 3]])
    return {"identity": np.arange(B, dtype=np.uint32), "reversed": np.arange(B, dtype=np.uint32)[::-1].copy(), "permutation": perm,
            "every_third": np.arange(0, B, 3, dtype=np.uint32), "empty": np.zeros(0, np.uint32), "past_the_batch": mixed[rng.permutation(len(mixed))]}


def poisoned(B, max_spans=MAX_SPANS):
    return np.full(B, P64, np.uint64), np.full(B, P32, np.uint32), np.full((B, max_spans), P64, np.uint64)


def check_selected(got, full, sel, B):
    """selected entries = the unselected call's, every other entry = the poison (run slots included)"""
    st, cnt, sp = got
    fst, fcnt, fsp = full
    mask = np.zeros(B, bool)
    mask[sel[sel < B]] = True
    assert np.array_equal(st[mask], fst[mask]) and np.array_equal(cnt[mask], fcnt[mask])
    assert hra.decode_spans(cnt[mask], sp[mask]) == hra.decode_spans(fcnt[mask], fsp[mask])
    assert (st[~mask] == P64).all() and (cnt[~mask] == P32).all() and (sp[~mask] == P64).all()


def test_symbols_are_exported_and_bound():
    for name in ("hrx_match_selected_device", "hrx_match_selected_host"):
        fn = getattr(hra.lib, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    assert hra.LAYOUT_INPUT_SELECTED == 16
    assert callable(hra.RegexVerifyConfig.match_selected) and callable(hra.RegexVerifyConfig.match_selected_host)


@pytest.mark.parametrize("name,names", CFGS, ids=[c[0] for c in CFGS])
def test_selected_entries_equal_the_unselected_call(name, names):
    cfg = _cfg(names, M)
    chars, lens = edge_batch()
    B = len(lens)
    values, offsets = column(chars, lens)
    full_p = cfg.match_batch_host(chars, lens, max_spans=MAX_SPANS)
    full_r = cfg.match_batch_host_ragged(values, offsets, max_spans=MAX_SPANS)
    assert int(full_r[0][7]) == BAD_LENGTH and int((full_p[0] & np.uint64(0xff) == BAD_LENGTH).sum()) == 3
    for kind, sel in selections(B).items():
        got = cfg.match_selected_host(chars, sel, lens=lens, max_spans=MAX_SPANS, out=poisoned(B))
        check_selected(got, full_p, sel, B)
        got = cfg.match_selected_host(values, sel, offsets=offsets, max_spans=MAX_SPANS, out=poisoned(B))
        check_selected(got, full_r, sel, B)


def test_status_only_and_counts_only():
    cfg = _cfg(CFG_1, M)
    chars, lens = edge_batch()
    B = len(lens)
    sel = np.arange(1, B, 2, dtype=np.uint32)
    full = cfg.match_batch_host(chars, lens, max_spans=MAX_SPANS)
    st, cnt, _ = cfg.match_selected_host(chars, sel, lens=lens, max_spans=0, out=(poisoned(B)[0], poisoned(B)[1], np.zeros((B, 0), np.uint64)))
    assert np.array_equal(st[1::2], full[0][1::2]) and np.array_equal(cnt[1::2], full[1][1::2])
    assert (st[0::2] == P64).all() and (cnt[0::2] == P32).all()


def test_a_string_longer_than_its_slot_has_no_valid_length():
    """lens[b] > src_stride: kStatusBadLength, count 0, none of its bytes read (the unselected host entry refuses such a batch; every other string
    gets what that entry gives the batch with this length replaced by M + 1)"""
    Ms, stride = 64, 32
    cfg = _cfg(CFG_1, Ms)
    chars = np.zeros((4, stride), np.uint8)
    hit = np.frombuffer(b"email was meant for @y.", np.uint8)
    chars[:, :len(hit)] = hit
    lens = np.array([23, 40, 32, 70], np.uint32)
    with pytest.raises(hra.HrxError):
        cfg.match_batch_host(chars, lens, max_spans=4)
    ref = cfg.match_batch_host(chars, np.array([23, Ms + 1, 32, 70], np.uint32), max_spans=4)
    got = cfg.match_selected_host(chars, np.array([3, 1, 0, 2], np.uint32), lens=lens, max_spans=4, out=poisoned(4, 4))
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert int(got[0][1]) == BAD_LENGTH and int(got[1][1]) == 0 and int(got[0][3]) == BAD_LENGTH and int(got[1][0]) == 1
    assert (got[2][1] == P64).all() and (got[2][3] == P64).all()


def test_argument_errors():
    cfg = _cfg(CFG_1, M)
    ctx = cfg._need_ctx()
    L = hra.lib
    chars, lens = edge_batch()
    B, stride = chars.shape
    values, offsets = column(chars, lens)
    sel = np.arange(B, dtype=np.uint32)
    st, cnt, sp = poisoned(B)
    p = lambda a: a.ctypes.data
    out = (p(st), p(cnt), p(sp), MAX_SPANS)
    host = lambda layout, src, sstride, ln, off, s, n_sel, o=out, m=M: L.hrx_match_selected_host(ctx, layout, src, sstride, ln, off, B, s, n_sel, m, *o)
    dev = lambda layout, src, sstride, ln, off, s, n_sel, o=out: L.hrx_match_selected_device(ctx, layout, src, sstride, ln, off, B, s, n_sel, M, *o, None)
    assert host(hra.LAYOUT_STRING_MAJOR, p(chars), stride, p(lens), None, p(sel), B) == hra.HRX_OK
    assert host(hra.LAYOUT_INPUT_RAGGED, p(values), 0, None, p(offsets), p(sel), B) == hra.HRX_OK
    # position-major input is refused, by both entries, whatever else is passed
    assert host(hra.LAYOUT_INPUT_POSITION_MAJOR, p(chars), stride, p(lens), None, p(sel), B) == hra.HRX_ERR_ARG
    assert dev(hra.LAYOUT_INPUT_POSITION_MAJOR, p(chars), stride, p(lens), None, p(sel), B) == hra.HRX_ERR_ARG
    assert host(hra.LAYOUT_INPUT_SELECTED, p(chars), stride, p(lens), None, p(sel), B) == hra.HRX_ERR_ARG
    # NULL sel with n_sel > 0; n_sel == 0 needs none
    assert host(hra.LAYOUT_STRING_MAJOR, p(chars), stride, p(lens), None, None, B) == hra.HRX_ERR_ARG
    assert dev(hra.LAYOUT_INPUT_RAGGED, p(values), 0, None, p(offsets), None, 1) == hra.HRX_ERR_ARG
    assert host(hra.LAYOUT_STRING_MAJOR, p(chars), stride, p(lens), None, None, 0) == hra.HRX_OK
    # the source's own pointer of each layout, and the outputs
    assert host(hra.LAYOUT_STRING_MAJOR, p(chars), stride, None, p(offsets), p(sel), B) == hra.HRX_ERR_ARG
    assert host(hra.LAYOUT_INPUT_RAGGED, p(values), 0, p(lens), None, p(sel), B) == hra.HRX_ERR_ARG
    assert host(hra.LAYOUT_STRING_MAJOR, None, stride, p(lens), None, p(sel), B) == hra.HRX_ERR_ARG
    assert host(hra.LAYOUT_STRING_MAJOR, p(chars), stride, p(lens), None, p(sel), B, (None, p(cnt), p(sp), MAX_SPANS)) == hra.HRX_ERR_ARG
    assert host(hra.LAYOUT_STRING_MAJOR, p(chars), stride, p(lens), None, p(sel), B, (p(st), p(cnt), None, MAX_SPANS)) == hra.HRX_ERR_ARG
    assert host(hra.LAYOUT_INPUT_RAGGED, p(values), 0, None, p(offsets) + 4, p(sel), B) == hra.HRX_ERR_ARG          # offsets not 8-byte aligned
    assert host(hra.LAYOUT_STRING_MAJOR, p(chars), stride, p(lens), None, p(sel) + 1, B - 1) == hra.HRX_ERR_ARG      # sel not 4-byte aligned
    # max_spans > 2^16, M out of range
    assert host(hra.LAYOUT_STRING_MAJOR, p(chars), stride, p(lens), None, p(sel), B, (p(st), p(cnt), p(sp), (1 << 16) + 1)) == hra.HRX_ERR_ARG
    assert host(hra.LAYOUT_STRING_MAJOR, p(chars), stride, p(lens), None, p(sel), B, m=0) == hra.HRX_ERR_ARG
    # the device entry: a misaligned src is an argument error, reported before the host-only context's own refusal
    buf = np.zeros(values.size + 32, np.uint8)
    a16 = (-p(buf)) % 16
    assert dev(hra.LAYOUT_INPUT_RAGGED, p(buf) + a16 + 1, 0, None, p(offsets), p(sel), B) == hra.HRX_ERR_ARG
    assert dev(hra.LAYOUT_STRING_MAJOR, p(buf) + a16 + 8, stride, p(lens), None, p(sel), B) == hra.HRX_ERR_ARG
    assert dev(hra.LAYOUT_STRING_MAJOR, p(buf) + a16, stride + 8, p(lens), None, p(sel), B) == hra.HRX_ERR_ARG
    assert dev(hra.LAYOUT_INPUT_RAGGED, p(buf) + a16, 0, None, p(offsets), p(sel), B) == hra.HRX_ERR_HIP            # refused, not run on the host
    assert L.hrx_match_selected_host(None, hra.LAYOUT_STRING_MAJOR, p(chars), stride, p(lens), None, B, p(sel), B, M, *out) == hra.HRX_ERR_ARG
    # the Python wrapper wants exactly one of lens and offsets
    with pytest.raises(hra.HrxError):
        cfg.match_selected_host(chars, sel)
    with pytest.raises(hra.HrxError):
        cfg.match_selected_host(chars, sel, lens=lens, offsets=offsets)


def test_describe_names_the_selected_launch():
    RAG, PAD = SEL | hra.LAYOUT_INPUT_RAGGED, SEL | hra.LAYOUT_STRING_MAJOR
    for names, lds in ((CFG_1, 31744), (CFG_23, 37888), (CFG_H3, 76800)):
        cfg, D = _cfg(names, 1024), len(names)
        assert cfg.describe_match(65536, layout=RAG) == "hrx::match_selected_kernel<%d, false, false, hrx::RaggedSrc> grid=persistent threads=256 lds=%d" % (D, lds)
        assert cfg.describe_match(65536, layout=PAD) == "hrx::match_selected_kernel<%d, false, false, hrx::PaddedSrc> grid=persistent threads=256 lds=%d" % (D, lds)
        assert cfg.describe_match(300, layout=RAG) == "hrx::match_selected_kernel<%d, false, false, hrx::RaggedSrc> grid=persistent threads=64 lds=%d" % (D, lds)
    cfg4 = _cfg(CFG_H4, 1024)
    # four defs: via rows, the staged bytes counted as for ragged input (41382 strings a slice, as HRX_LAYOUT_INPUT_RAGGED)
    assert cfg4.describe_match(65536, layout=PAD) == ("via rows, 2 slice(s) of 41382 strings: hrx::selected_slice_kernel<hrx::PaddedSrc> + "
                                                      "hrx::witness_pmd_kernel<4, true, true, false> grid=256 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_selected_kernel")
    assert cfg4.describe_match(300, layout=RAG) == ("via rows, 1 slice(s) of 300 strings: hrx::selected_slice_kernel<hrx::RaggedSrc> + "
                                                    "hrx::witness_pmd_kernel<4, true, true, false> grid=5 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_selected_kernel")
    # the flag goes with the two source layouts only
    for bad in (SEL | hra.LAYOUT_INPUT_POSITION_MAJOR, SEL | hra.LAYOUT_POSITION_MAJOR, SEL | 4):
        with pytest.raises(hra.HrxError):
            cfg4.describe_match(300, layout=bad)
    buf = C.create_string_buffer(4096)
    assert hra.lib.hrx_describe_match(cfg4._defs.h, RAG, 4500, 32768, 256, buf, 4096) == hra.HRX_OK
    assert buf.value.decode().startswith("via rows, 4 slice(s) of 1293 strings: hrx::selected_slice_kernel<hrx::RaggedSrc> + ")


def test_unselected_describe_texts_are_what_they_were():
    want = [
        ((CFG_1, 0, 65536, 1024), "hrx::match_lane_kernel<1, false, false> grid=256 threads=256 lds=31744"),
        ((CFG_1, 8, 300, 1024), "hrx::match_ragged_kernel<1, false, false> grid=persistent threads=64 lds=31744"),
        ((CFG_1, 8, 4500, 32768), "via rows, 2 slice(s) of 3510 strings: hrx::ragged_slice_kernel + hrx::witness_pm_kernel<1, false, false, false, false, false> grid=256 "
                                 "waves=12 ring=4 lds=138752 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind "
                                 "+ hrx::spans_from_masked_pm_kernel"),
        ((CFG_23, 2, 65536, 1024), "hrx::match_lane_kernel<2, false, false> grid=256 threads=256 lds=37888"),
        ((CFG_H3, 8, 65536, 1024), "hrx::match_ragged_kernel<3, false, false> grid=persistent threads=256 lds=76800"),
        ((CFG_H4, 0, 65536, 1024), "via rows, 2 slice(s) of 43690 strings: hrx::witness_pmd_kernel<4, true, true, false> grid=256 waves=6 ring=4 lds=93888 + "
                                  "hrx::spans_from_masked_pm_kernel"),
        ((CFG_H4, 2, 4500, 32768), "via rows, 4 slice(s) of 1365 strings: hrx::pm_input_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=22 waves=6 ring=4 "
                                  "lds=93888 + hrx::spans_from_masked_pm_kernel"),
        ((CFG_H4, 8, 300, 1024), "via rows, 1 slice(s) of 300 strings: hrx::ragged_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=5 waves=6 ring=4 lds=93888 "
                                "+ hrx::spans_from_masked_pm_kernel"),
    ]
    for i, ((names, layout, B, Mx), text) in enumerate(want):
        buf = C.create_string_buffer(4096)
        assert hra.lib.hrx_describe_match(_cfg(names, Mx)._defs.h, layout, B, Mx, 256, buf, 4096) == hra.HRX_OK
        assert buf.value.decode() == text, i
    # the layouts refused before are refused still
    for bad in (1, 4, 3, 32):
        assert hra.lib.hrx_describe_match(_cfg(CFG_1, 1024)._defs.h, bad, 300, 1024, 256, buf, 4096) == hra.HRX_ERR_ARG
