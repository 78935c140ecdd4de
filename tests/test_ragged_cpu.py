"""Ragged input (include/hrx.h RAGGED: values + B + 1 offsets) on host-only contexts: hrx_match_batch_host_ragged bit for bit what
hrx_match_batch_host gives the same strings padded, and what the oracle's witness reveals; offset edge cases (offsets[0] != 0, odd byte
offsets, slices of a larger column, decreasing offsets); argument checks; the kernel hrx_describe_match names for HRX_LAYOUT_INPUT_RAGGED."""
import os

import numpy as np
import pytest

import halo2_regex_amd as hra
from halo2_regex_amd import synth
from oracle_lib import OracleDefs
from test_match_cpu import CFG_1, CFG_23, CFG_H3, CFG_H4, _cfg, rle_masked

BAD_LENGTH = 3


def _big_dfa_cfg(M):
    """the 256-state random DFA (configs[4] stand-in): its narrow table does not fit LDS, the HALF table does"""
    a_txt, sub = synth.random_dfa(256, seed=2, alphabet=np.arange(256, dtype=np.uint8), n_substr_pairs=40)
    defs = [hra.RegexDefs(hra.AllstrRegexDef(a_txt), [hra.SubstrRegexDef(sub)])]
    return defs, (a_txt, sub)


def _padded(strings, M):
    """the padded form of the same strings: chars [B][stride], lens (strings longer than M keep a length > M)"""
    stride = max(16, -(-max([len(x) for x in strings] + [M + 1]) // 16) * 16)
    chars = np.zeros((len(strings), stride), np.uint8)
    lens = np.zeros(len(strings), np.uint32)
    for b, x in enumerate(strings):
        chars[b, :len(x)] = np.frombuffer(bytes(x), np.uint8)
        lens[b] = len(x)
    return chars, lens


def _column(strings, lead=0, seed=0):
    """values + offsets with `lead` junk bytes in front (offsets[0] != 0; odd lengths make odd offsets) and junk after the last string"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, lead, dtype=np.uint8).tobytes() + b"".join(bytes(x) for x in strings)
    offsets = np.zeros(len(strings) + 1, np.uint64)
    np.cumsum([len(x) for x in strings], out=offsets[1:])
    values = rng.integers(0, 256, -(-len(raw) // 16) * 16 + 16, dtype=np.uint8)
    values[:len(raw)] = np.frombuffer(raw, np.uint8)
    return values, offsets + np.uint64(lead)


def _strings(chars, lens):
    return [chars[b, :int(lens[b])].tobytes() for b in range(len(lens))]


def check_ragged(oracle, names, strings, M, values=None, offsets=None, cfg=None, o=None, max_spans=64):
    cfg = cfg or _cfg(names, M)
    if values is None:
        values, offsets = hra.pack_strings(strings)
    chars, lens = _padded(strings, M)
    st, cnt, sp = cfg.match_batch_host_ragged(values, offsets, max_spans=max_spans)
    pst, pcnt, psp = cfg.match_batch_host(chars, lens, max_spans=max_spans)
    assert np.array_equal(st, pst) and np.array_equal(cnt, pcnt)
    assert hra.decode_spans(cnt, sp) == hra.decode_spans(pcnt, psp)
    if o is not False:
        o = o or OracleDefs.from_files(oracle, names)
        _, omsk, ost = o.witness_batch(chars, lens, M, threads=8)
        assert np.array_equal(st, ost)
        ecnt, eruns = rle_masked(omsk, lens, ost)
        assert cnt.tolist() == ecnt
        got = hra.decode_spans(cnt, sp)
        assert all(got[b] == eruns[b][:max_spans] for b in range(len(strings)))
    return st, cnt, sp


CFGS = [("regex1", CFG_1, 1024), ("regex23", CFG_23, 2048), ("headers3", CFG_H3, 1024), ("headers4", CFG_H4, 1024)]


@pytest.mark.parametrize("name,names,M", CFGS, ids=[c[0] for c in CFGS])
def test_synth_ragged_mix(oracle, name, names, M):
    chars, lens = synth.ragged(300, M, seed=11)
    check_ragged(oracle, names, _strings(chars, lens), M)


@pytest.mark.parametrize("name,names,M", CFGS, ids=[c[0] for c in CFGS])
def test_edge_lengths_offsets_and_slices(oracle, name, names, M):
    rng = np.random.default_rng(5)
    body, _ = synth.reveal_stress(64, M + 1, seed=3)
    edge = [0, 1, 15, 16, 17, 63, 64, 65, M - 1, M, M + 1]
    strings = []
    for k, n in enumerate(edge * 3):
        row = body[k % 64]
        strings.append(bytes(row[:n]) if n <= len(row) else bytes(row) + b"x" * (n - len(row)))
    rng.shuffle(strings)
    o = OracleDefs.from_files(oracle, names)
    cfg = _cfg(names, M)
    check_ragged(oracle, names, strings, M, cfg=cfg, o=o)
    for lead in (7, 3, 16, 1):                                              # offsets[0] != 0, odd byte offsets
        values, offsets = _column(strings, lead, seed=lead)
        check_ragged(oracle, names, strings, M, values, offsets, cfg=cfg, o=o)
    values, offsets = _column(strings, 9, seed=1)                           # a slice of a larger column: offsets + begin
    for lo, hi in ((5, 20), (0, 1), (17, len(strings))):
        check_ragged(oracle, names, strings[lo:hi], M, values, offsets[lo:hi + 1], cfg=cfg, o=o)
    st, cnt, _ = cfg.match_batch_host_ragged(values, offsets)
    assert [int(s) & 0xff for s, x in zip(st, strings) if len(x) > M] == [BAD_LENGTH] * 3


def test_half_table_dfa(oracle):
    M = 1024
    defs, (a_txt, sub) = _big_dfa_cfg(M)
    cfg = hra.RegexVerifyConfig.configure(M, defs, device=hra.HRX_DEVICE_NONE)
    chars, lens = synth.ragged(200, M, seed=4, alphabet=np.arange(256, dtype=np.uint8))
    strings = _strings(chars, lens)
    o = OracleDefs(oracle, [(a_txt.encode(), [sub.encode()])])
    values, offsets = _column(strings, 5)
    check_ragged(oracle, None, strings, M, values, offsets, cfg=cfg, o=o)
    assert cfg.describe_match(65536, layout=hra.LAYOUT_INPUT_RAGGED).startswith("hrx::match_ragged_kernel<1, false, true> ")


def test_planted_pattern_across_a_string_boundary(oracle):
    """the bytes after a string's end complete a match: the walk must stop at n_b (each prefix gives what its padded copy gives)"""
    M = 256
    hit = b"email was meant for @bob."
    strings = [hit[:k] for k in range(len(hit) + 1)] + [hit]
    values = np.zeros(1024, np.uint8)
    raw = b"".join(hit for _ in strings)
    values[:len(raw)] = np.frombuffer(raw, np.uint8)
    # string k = the first k bytes of a copy of hit, the rest of that copy follows it in values
    cfg = _cfg(CFG_1, M)
    counts = []
    for k, x in enumerate(strings):
        o = np.array([len(hit) * k, len(hit) * k + len(x)], np.uint64)
        st, cnt, _ = cfg.match_batch_host_ragged(values, o)
        pst, pcnt, _ = cfg.match_batch_host(*_padded([x], M))
        assert int(st[0]) == int(pst[0]) and int(cnt[0]) == int(pcnt[0])
        counts.append(int(cnt[0]))
    assert counts[-1] == 1 and counts[:21] == [0] * 21           # (nothing before the '@')
    check_ragged(oracle, CFG_1, strings, M, *_column(strings))


def test_decreasing_offsets_bad_arguments_and_empty_batch():
    M = 64
    cfg = _cfg(CFG_1, M)
    values = np.frombuffer(b"email was meant for @y." + b"\x00" * 9, np.uint8).copy()
    offsets = np.array([0, 23, 10, 23, 23], np.uint64)          # string 1 decreases; 2: 13 bytes; 3: empty
    st, cnt, sp = cfg.match_batch_host_ragged(values, offsets)
    assert int(st[1]) == BAD_LENGTH and int(cnt[1]) == 0
    assert int(st[0]) & 0xff == 0 and int(cnt[0]) == 1
    assert int(st[3]) & 0xff == 0 and int(cnt[3]) == 0
    st, cnt, sp = cfg.match_batch_host_ragged(values, np.zeros(1, np.uint64))       # B = 0
    assert st.shape == (0,) and cnt.shape == (0,)
    import ctypes as C
    L = hra.lib
    st = np.zeros(4, np.uint64)
    cnt = np.zeros(4, np.uint32)
    sp = np.zeros(4 * 16, np.uint64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    ctx = cfg._need_ctx()
    assert L.hrx_match_batch_host_ragged(ctx, None, offsets.ctypes.data_as(C.POINTER(C.c_uint64)), 4, M, st.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         cnt.ctypes.data_as(C.POINTER(C.c_uint32)), sp.ctypes.data_as(C.POINTER(C.c_uint64)), 16) == hra.HRX_ERR_ARG
    assert L.hrx_match_batch_host_ragged(ctx, values.ctypes.data_as(C.POINTER(C.c_uint8)), None, 4, M, st.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         cnt.ctypes.data_as(C.POINTER(C.c_uint32)), sp.ctypes.data_as(C.POINTER(C.c_uint64)), 16) == hra.HRX_ERR_ARG
    raw = np.zeros(8 * 6, np.uint8)
    odd = (C.c_uint64 * 6).from_buffer(raw)                       # an offsets pointer off by one byte
    odd_ptr = C.cast(C.addressof(odd) + 1, C.POINTER(C.c_uint64))
    assert L.hrx_match_batch_host_ragged(ctx, values.ctypes.data_as(C.POINTER(C.c_uint8)), odd_ptr, 4, M, st.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         cnt.ctypes.data_as(C.POINTER(C.c_uint32)), sp.ctypes.data_as(C.POINTER(C.c_uint64)), 16) == hra.HRX_ERR_ARG
    # the device entries on a host-only context: refused, not run on the host
    assert L.hrx_match_batch_device_ragged(ctx, vp(values), vp(offsets), 4, M, vp(st), vp(cnt), vp(sp), 16, None) != hra.HRX_OK
    assert L.hrx_ragged_to_position_major_device(ctx, vp(values), vp(offsets), 4, 64, vp(sp), vp(cnt), None) != hra.HRX_OK


def test_describe_match_ragged_names_the_kernels():
    def desc(names, B, M, flags=None):
        if flags is not None:
            os.environ["HRX_DEBUG_FLAGS"] = str(flags)
        try:
            cfg = _cfg(names, M)
        finally:
            os.environ.pop("HRX_DEBUG_FLAGS", None)
        return cfg.describe_match(B, layout=hra.LAYOUT_INPUT_RAGGED)
    for names in (CFG_1, CFG_23, CFG_H3):
        D = len(names)
        assert desc(names, 65536, 1024).startswith("hrx::match_ragged_kernel<%d, false, false> grid=persistent " % D)
        for flags, args in ((0x80000, "false, false"), (0x200000, "false, false"), (0x400000, "false, true"), (0x2000, "false, true"), (0x40000, "true, false")):
            assert desc(names, 65536, 1024, flags).startswith("hrx::match_ragged_kernel<%d, %s> " % (D, args)), (D, flags)
        v = desc(names, 65536, 1024, 1 << 32)
        assert v.startswith("via rows") and "hrx::ragged_slice_kernel" in v and "spans_from_masked_pm_kernel" in v
    d4 = desc(CFG_H4, 65536, 2048)
    assert d4.startswith("via rows") and "hrx::ragged_slice_kernel" in d4 and "witness_pmd_kernel<4" in d4
    assert desc(CFG_1, 8192, 32768).startswith("via rows")                           # few long strings: the chunked witness
    # the padded layouts' text does not change
    assert _cfg(CFG_1, 1024).describe_match(65536).startswith("hrx::match_lane_kernel<1, false, false> grid=256 threads=256 ")


def test_describe_match_text_in_full():
    """hrx_describe_match, the complete text (DESCRIBE_MATCH_TEXT below, recorded before the padded and the ragged form came to share their via-rows
    arithmetic): the fused kernel and its launch shape, the slice counts and sizes of both via-rows forms, the gather decision"""
    import ctypes as C
    cfgs = {"regex1": CFG_1, "regex23": CFG_23, "headers3": CFG_H3, "headers4": CFG_H4}
    built = {}
    assert len(DESCRIBE_MATCH_TEXT) == 4 * 3 * 4 * 2
    for (name, layout, B, M, via_rows), want in DESCRIBE_MATCH_TEXT.items():
        cfg = built.get((name, M)) or built.setdefault((name, M), _cfg(cfgs[name], M))
        buf = C.create_string_buffer(4096)
        if via_rows:
            os.environ["HRX_DEBUG_FLAGS"] = str(1 << 32)
        try:
            rc = hra.lib.hrx_describe_match(cfg._defs.h, layout, B, M, 256, buf, 4096)
        finally:
            os.environ.pop("HRX_DEBUG_FLAGS", None)
        assert rc == hra.HRX_OK and buf.value.decode() == want, (name, layout, B, M, via_rows)


def test_pack_strings_and_match_strings_round_trip(oracle):
    strings = [b"", b"a", b"email was meant for @y.", bytes(range(256)), b"x" * 1000, b"email was meant for @bob. tail"]
    values, offsets = hra.pack_strings(strings)
    assert values.dtype == np.uint8 and offsets.dtype == np.uint64 and len(values) % 16 == 0 and len(offsets) == len(strings) + 1
    assert [values[int(offsets[b]):int(offsets[b + 1])].tobytes() for b in range(len(strings))] == strings
    assert hra.pack_strings([])[1].tolist() == [0]
    M = 1024
    cfg = _cfg(CFG_1, M)
    st, cnt, sp = cfg.match_strings(strings)
    pst, pcnt, psp = cfg.match_batch_host(*_padded(strings, M))
    assert np.array_equal(st, pst) and np.array_equal(cnt, pcnt)
    got = hra.revealed_substrings_ragged(values, offsets, st, cnt, sp)
    assert got[2] == [(1, 21, b"y")] and got[5] == [(1, 21, b"bob")]
    assert got == hra.revealed_substrings(*_padded(strings, M), st, cnt, sp)
    check_ragged(oracle, CFG_1, strings, M)


# (config, layout, B, M, HRX_DEBUG_FLAGS bit 32) -> hrx_describe_match with num_cus = 256.  Layouts: 0 string-major, 2 position-major input, 8 ragged
DESCRIBE_MATCH_TEXT = {
    ('regex1', 0, 65536, 1024, False): 'hrx::match_lane_kernel<1, false, false> grid=256 threads=256 lds=31744',
    ('regex1', 0, 65536, 1024, True): 'via rows, 1 slice(s) of 65536 strings: hrx::witness_pm_kernel<1, false, false, false, false, false> grid=256 waves=12 ring=4 lds=138752 + hrx::spans_from_masked_pm_kernel',
    ('regex1', 2, 65536, 1024, False): 'hrx::match_lane_kernel<1, false, false> grid=256 threads=256 lds=31744',
    ('regex1', 2, 65536, 1024, True): 'via rows, 1 slice(s) of 65536 strings: hrx::witness_pm_kernel<1, false, false, false, false, false> grid=256 waves=12 ring=4 lds=138752 + hrx::spans_from_masked_pm_kernel',
    ('regex1', 8, 65536, 1024, False): 'hrx::match_ragged_kernel<1, false, false> grid=persistent threads=256 lds=31744',
    ('regex1', 8, 65536, 1024, True): 'via rows, 1 slice(s) of 65536 strings: hrx::ragged_slice_kernel + hrx::witness_pm_kernel<1, false, false, false, false, false> grid=256 waves=12 ring=4 lds=138752 + hrx::spans_from_masked_pm_kernel',
    ('regex1', 0, 300, 1024, False): 'hrx::match_lane_kernel<1, false, false> grid=5 threads=64 lds=31744',
    ('regex1', 0, 300, 1024, True): 'via rows, 1 slice(s) of 300 strings: hrx::witness_pp_kernel grid=5 waves=3 ring=4 lds=117056 + hrx::spans_from_masked_pm_kernel',
    ('regex1', 2, 300, 1024, False): 'hrx::match_lane_kernel<1, false, false> grid=5 threads=64 lds=31744',
    ('regex1', 2, 300, 1024, True): 'via rows, 1 slice(s) of 300 strings: hrx::witness_pp_kernel grid=5 waves=3 ring=4 lds=117056 + hrx::spans_from_masked_pm_kernel',
    ('regex1', 8, 300, 1024, False): 'hrx::match_ragged_kernel<1, false, false> grid=persistent threads=64 lds=31744',
    ('regex1', 8, 300, 1024, True): 'via rows, 1 slice(s) of 300 strings: hrx::ragged_slice_kernel + hrx::witness_pp_kernel grid=5 waves=3 ring=4 lds=117056 + hrx::spans_from_masked_pm_kernel',
    ('regex1', 0, 4500, 32768, False): 'via rows, 2 slice(s) of 4096 strings: hrx::witness_pm_kernel<1, false, false, false, false, false> grid=256 waves=12 ring=4 lds=138752 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex1', 0, 4500, 32768, True): 'via rows, 2 slice(s) of 4096 strings: hrx::witness_pm_kernel<1, false, false, false, false, false> grid=256 waves=12 ring=4 lds=138752 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex1', 2, 4500, 32768, False): 'via rows, 2 slice(s) of 4096 strings: hrx::pm_input_slice_kernel + hrx::witness_pm_kernel<1, false, false, false, false, false> grid=256 waves=12 ring=4 lds=138752 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex1', 2, 4500, 32768, True): 'via rows, 2 slice(s) of 4096 strings: hrx::pm_input_slice_kernel + hrx::witness_pm_kernel<1, false, false, false, false, false> grid=256 waves=12 ring=4 lds=138752 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex1', 8, 4500, 32768, False): 'via rows, 2 slice(s) of 3510 strings: hrx::ragged_slice_kernel + hrx::witness_pm_kernel<1, false, false, false, false, false> grid=256 waves=12 ring=4 lds=138752 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex1', 8, 4500, 32768, True): 'via rows, 2 slice(s) of 3510 strings: hrx::ragged_slice_kernel + hrx::witness_pm_kernel<1, false, false, false, false, false> grid=256 waves=12 ring=4 lds=138752 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex1', 0, 8192, 32768, False): 'via rows, 2 slice(s) of 4096 strings: hrx::witness_pm_kernel<1, false, false, false, false, false> grid=256 waves=12 ring=4 lds=138752 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex1', 0, 8192, 32768, True): 'via rows, 2 slice(s) of 4096 strings: hrx::witness_pm_kernel<1, false, false, false, false, false> grid=256 waves=12 ring=4 lds=138752 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex1', 2, 8192, 32768, False): 'via rows, 2 slice(s) of 4096 strings: hrx::pm_input_slice_kernel + hrx::witness_pm_kernel<1, false, false, false, false, false> grid=256 waves=12 ring=4 lds=138752 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex1', 2, 8192, 32768, True): 'via rows, 2 slice(s) of 4096 strings: hrx::pm_input_slice_kernel + hrx::witness_pm_kernel<1, false, false, false, false, false> grid=256 waves=12 ring=4 lds=138752 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex1', 8, 8192, 32768, False): 'via rows, 3 slice(s) of 3510 strings: hrx::ragged_slice_kernel + hrx::witness_pm_kernel<1, false, false, false, false, false> grid=256 waves=12 ring=4 lds=138752 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex1', 8, 8192, 32768, True): 'via rows, 3 slice(s) of 3510 strings: hrx::ragged_slice_kernel + hrx::witness_pm_kernel<1, false, false, false, false, false> grid=256 waves=12 ring=4 lds=138752 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex23', 0, 65536, 1024, False): 'hrx::match_lane_kernel<2, false, false> grid=256 threads=256 lds=37888',
    ('regex23', 0, 65536, 1024, True): 'via rows, 1 slice(s) of 65536 strings: hrx::witness_pm_kernel<2, false, true, false, false, false> grid=256 waves=12 ring=4 lds=144896 + hrx::spans_from_masked_pm_kernel',
    ('regex23', 2, 65536, 1024, False): 'hrx::match_lane_kernel<2, false, false> grid=256 threads=256 lds=37888',
    ('regex23', 2, 65536, 1024, True): 'via rows, 1 slice(s) of 65536 strings: hrx::witness_pm_kernel<2, false, true, false, false, false> grid=256 waves=12 ring=4 lds=144896 + hrx::spans_from_masked_pm_kernel',
    ('regex23', 8, 65536, 1024, False): 'hrx::match_ragged_kernel<2, false, false> grid=persistent threads=256 lds=37888',
    ('regex23', 8, 65536, 1024, True): 'via rows, 1 slice(s) of 65536 strings: hrx::ragged_slice_kernel + hrx::witness_pm_kernel<2, false, true, false, false, false> grid=256 waves=12 ring=4 lds=144896 + hrx::spans_from_masked_pm_kernel',
    ('regex23', 0, 300, 1024, False): 'hrx::match_lane_kernel<2, false, false> grid=5 threads=64 lds=37888',
    ('regex23', 0, 300, 1024, True): 'via rows, 1 slice(s) of 300 strings: hrx::witness_pmd_kernel<2, false, false, false> grid=5 waves=3 ring=4 lds=66752 + hrx::spans_from_masked_pm_kernel',
    ('regex23', 2, 300, 1024, False): 'hrx::match_lane_kernel<2, false, false> grid=5 threads=64 lds=37888',
    ('regex23', 2, 300, 1024, True): 'via rows, 1 slice(s) of 300 strings: hrx::witness_pmd_kernel<2, false, false, false> grid=5 waves=3 ring=4 lds=66752 + hrx::spans_from_masked_pm_kernel',
    ('regex23', 8, 300, 1024, False): 'hrx::match_ragged_kernel<2, false, false> grid=persistent threads=64 lds=37888',
    ('regex23', 8, 300, 1024, True): 'via rows, 1 slice(s) of 300 strings: hrx::ragged_slice_kernel + hrx::witness_pmd_kernel<2, false, false, false> grid=5 waves=3 ring=4 lds=66752 + hrx::spans_from_masked_pm_kernel',
    ('regex23', 0, 4500, 32768, False): 'via rows, 2 slice(s) of 2457 strings: hrx::witness_pm_kernel<2, false, true, false, false, false> grid=256 waves=12 ring=4 lds=144896 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex23', 0, 4500, 32768, True): 'via rows, 2 slice(s) of 2457 strings: hrx::witness_pm_kernel<2, false, true, false, false, false> grid=256 waves=12 ring=4 lds=144896 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex23', 2, 4500, 32768, False): 'via rows, 2 slice(s) of 2457 strings: hrx::pm_input_slice_kernel + hrx::witness_pm_kernel<2, false, true, false, false, false> grid=256 waves=12 ring=4 lds=144896 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex23', 2, 4500, 32768, True): 'via rows, 2 slice(s) of 2457 strings: hrx::pm_input_slice_kernel + hrx::witness_pm_kernel<2, false, true, false, false, false> grid=256 waves=12 ring=4 lds=144896 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex23', 8, 4500, 32768, False): 'via rows, 3 slice(s) of 2234 strings: hrx::ragged_slice_kernel + hrx::witness_pm_kernel<2, false, true, false, false, false> grid=256 waves=12 ring=4 lds=144896 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex23', 8, 4500, 32768, True): 'via rows, 3 slice(s) of 2234 strings: hrx::ragged_slice_kernel + hrx::witness_pm_kernel<2, false, true, false, false, false> grid=256 waves=12 ring=4 lds=144896 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex23', 0, 8192, 32768, False): 'via rows, 4 slice(s) of 2457 strings: hrx::witness_pm_kernel<2, false, true, false, false, false> grid=256 waves=12 ring=4 lds=144896 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex23', 0, 8192, 32768, True): 'via rows, 4 slice(s) of 2457 strings: hrx::witness_pm_kernel<2, false, true, false, false, false> grid=256 waves=12 ring=4 lds=144896 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex23', 2, 8192, 32768, False): 'via rows, 4 slice(s) of 2457 strings: hrx::pm_input_slice_kernel + hrx::witness_pm_kernel<2, false, true, false, false, false> grid=256 waves=12 ring=4 lds=144896 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex23', 2, 8192, 32768, True): 'via rows, 4 slice(s) of 2457 strings: hrx::pm_input_slice_kernel + hrx::witness_pm_kernel<2, false, true, false, false, false> grid=256 waves=12 ring=4 lds=144896 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex23', 8, 8192, 32768, False): 'via rows, 4 slice(s) of 2234 strings: hrx::ragged_slice_kernel + hrx::witness_pm_kernel<2, false, true, false, false, false> grid=256 waves=12 ring=4 lds=144896 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('regex23', 8, 8192, 32768, True): 'via rows, 4 slice(s) of 2234 strings: hrx::ragged_slice_kernel + hrx::witness_pm_kernel<2, false, true, false, false, false> grid=256 waves=12 ring=4 lds=144896 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('headers3', 0, 65536, 1024, False): 'hrx::match_lane_kernel<3, false, false> grid=256 threads=256 lds=76800',
    ('headers3', 0, 65536, 1024, True): 'via rows, 2 slice(s) of 56173 strings: hrx::witness_pm_kernel<3, false, true, false, false, false> grid=220 waves=12 ring=2 lds=151040 + hrx::spans_from_masked_pm_kernel',
    ('headers3', 2, 65536, 1024, False): 'hrx::match_lane_kernel<3, false, false> grid=256 threads=256 lds=76800',
    ('headers3', 2, 65536, 1024, True): 'via rows, 2 slice(s) of 56173 strings: hrx::pm_input_slice_kernel + hrx::witness_pm_kernel<3, false, true, false, false, false> grid=220 waves=12 ring=2 lds=151040 + hrx::spans_from_masked_pm_kernel',
    ('headers3', 8, 65536, 1024, False): 'hrx::match_ragged_kernel<3, false, false> grid=persistent threads=256 lds=76800',
    ('headers3', 8, 65536, 1024, True): 'via rows, 2 slice(s) of 52415 strings: hrx::ragged_slice_kernel + hrx::witness_pm_kernel<3, false, true, false, false, false> grid=205 waves=12 ring=2 lds=151040 + hrx::spans_from_masked_pm_kernel',
    ('headers3', 0, 300, 1024, False): 'hrx::match_lane_kernel<3, false, false> grid=5 threads=64 lds=76800',
    ('headers3', 0, 300, 1024, True): 'via rows, 1 slice(s) of 300 strings: hrx::witness_pmd_kernel<3, false, false, false> grid=5 waves=4 ring=4 lds=117952 + hrx::spans_from_masked_pm_kernel',
    ('headers3', 2, 300, 1024, False): 'hrx::match_lane_kernel<3, false, false> grid=5 threads=64 lds=76800',
    ('headers3', 2, 300, 1024, True): 'via rows, 1 slice(s) of 300 strings: hrx::witness_pmd_kernel<3, false, false, false> grid=5 waves=4 ring=4 lds=117952 + hrx::spans_from_masked_pm_kernel',
    ('headers3', 8, 300, 1024, False): 'hrx::match_ragged_kernel<3, false, false> grid=persistent threads=64 lds=76800',
    ('headers3', 8, 300, 1024, True): 'via rows, 1 slice(s) of 300 strings: hrx::ragged_slice_kernel + hrx::witness_pmd_kernel<3, false, false, false> grid=5 waves=4 ring=4 lds=117952 + hrx::spans_from_masked_pm_kernel',
    ('headers3', 0, 4500, 32768, False): 'via rows, 3 slice(s) of 1755 strings: hrx::witness_pm_kernel<3, false, true, false, false, false> grid=224 waves=12 ring=2 lds=151040 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('headers3', 0, 4500, 32768, True): 'via rows, 3 slice(s) of 1755 strings: hrx::witness_pm_kernel<3, false, true, false, false, false> grid=224 waves=12 ring=2 lds=151040 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('headers3', 2, 4500, 32768, False): 'via rows, 3 slice(s) of 1755 strings: hrx::pm_input_slice_kernel + hrx::witness_pm_kernel<3, false, true, false, false, false> grid=224 waves=12 ring=2 lds=151040 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('headers3', 2, 4500, 32768, True): 'via rows, 3 slice(s) of 1755 strings: hrx::pm_input_slice_kernel + hrx::witness_pm_kernel<3, false, true, false, false, false> grid=224 waves=12 ring=2 lds=151040 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('headers3', 8, 4500, 32768, False): 'via rows, 3 slice(s) of 1638 strings: hrx::ragged_slice_kernel + hrx::witness_pm_kernel<3, false, true, false, false, false> grid=208 waves=12 ring=2 lds=151040 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('headers3', 8, 4500, 32768, True): 'via rows, 3 slice(s) of 1638 strings: hrx::ragged_slice_kernel + hrx::witness_pm_kernel<3, false, true, false, false, false> grid=208 waves=12 ring=2 lds=151040 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('headers3', 0, 8192, 32768, False): 'via rows, 5 slice(s) of 1755 strings: hrx::witness_pm_kernel<3, false, true, false, false, false> grid=224 waves=12 ring=2 lds=151040 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('headers3', 0, 8192, 32768, True): 'via rows, 5 slice(s) of 1755 strings: hrx::witness_pm_kernel<3, false, true, false, false, false> grid=224 waves=12 ring=2 lds=151040 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('headers3', 2, 8192, 32768, False): 'via rows, 5 slice(s) of 1755 strings: hrx::pm_input_slice_kernel + hrx::witness_pm_kernel<3, false, true, false, false, false> grid=224 waves=12 ring=2 lds=151040 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('headers3', 2, 8192, 32768, True): 'via rows, 5 slice(s) of 1755 strings: hrx::pm_input_slice_kernel + hrx::witness_pm_kernel<3, false, true, false, false, false> grid=224 waves=12 ring=2 lds=151040 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('headers3', 8, 8192, 32768, False): 'via rows, 6 slice(s) of 1638 strings: hrx::ragged_slice_kernel + hrx::witness_pm_kernel<3, false, true, false, false, false> grid=208 waves=12 ring=2 lds=151040 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('headers3', 8, 8192, 32768, True): 'via rows, 6 slice(s) of 1638 strings: hrx::ragged_slice_kernel + hrx::witness_pm_kernel<3, false, true, false, false, false> grid=208 waves=12 ring=2 lds=151040 chunked=32x16 tiles: hrx::spec_scout_kernel + hrx::spec_compose_kernel before, hrx::spec_stitch_kernel behind + hrx::spans_from_masked_pm_kernel',
    ('headers4', 0, 65536, 1024, False): 'via rows, 2 slice(s) of 43690 strings: hrx::witness_pmd_kernel<4, true, true, false> grid=256 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 0, 65536, 1024, True): 'via rows, 2 slice(s) of 43690 strings: hrx::witness_pmd_kernel<4, true, true, false> grid=256 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 2, 65536, 1024, False): 'via rows, 2 slice(s) of 43690 strings: hrx::pm_input_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=256 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 2, 65536, 1024, True): 'via rows, 2 slice(s) of 43690 strings: hrx::pm_input_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=256 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 8, 65536, 1024, False): 'via rows, 2 slice(s) of 41382 strings: hrx::ragged_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=256 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 8, 65536, 1024, True): 'via rows, 2 slice(s) of 41382 strings: hrx::ragged_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=256 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 0, 300, 1024, False): 'via rows, 1 slice(s) of 300 strings: hrx::witness_pmd_kernel<4, true, true, false> grid=5 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 0, 300, 1024, True): 'via rows, 1 slice(s) of 300 strings: hrx::witness_pmd_kernel<4, true, true, false> grid=5 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 2, 300, 1024, False): 'via rows, 1 slice(s) of 300 strings: hrx::witness_pmd_kernel<4, true, true, false> grid=5 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 2, 300, 1024, True): 'via rows, 1 slice(s) of 300 strings: hrx::witness_pmd_kernel<4, true, true, false> grid=5 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 8, 300, 1024, False): 'via rows, 1 slice(s) of 300 strings: hrx::ragged_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=5 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 8, 300, 1024, True): 'via rows, 1 slice(s) of 300 strings: hrx::ragged_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=5 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 0, 4500, 32768, False): 'via rows, 4 slice(s) of 1365 strings: hrx::witness_pmd_kernel<4, true, true, false> grid=22 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 0, 4500, 32768, True): 'via rows, 4 slice(s) of 1365 strings: hrx::witness_pmd_kernel<4, true, true, false> grid=22 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 2, 4500, 32768, False): 'via rows, 4 slice(s) of 1365 strings: hrx::pm_input_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=22 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 2, 4500, 32768, True): 'via rows, 4 slice(s) of 1365 strings: hrx::pm_input_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=22 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 8, 4500, 32768, False): 'via rows, 4 slice(s) of 1293 strings: hrx::ragged_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=21 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 8, 4500, 32768, True): 'via rows, 4 slice(s) of 1293 strings: hrx::ragged_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=21 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 0, 8192, 32768, False): 'via rows, 7 slice(s) of 1365 strings: hrx::witness_pmd_kernel<4, true, true, false> grid=22 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 0, 8192, 32768, True): 'via rows, 7 slice(s) of 1365 strings: hrx::witness_pmd_kernel<4, true, true, false> grid=22 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 2, 8192, 32768, False): 'via rows, 7 slice(s) of 1365 strings: hrx::pm_input_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=22 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 2, 8192, 32768, True): 'via rows, 7 slice(s) of 1365 strings: hrx::pm_input_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=22 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 8, 8192, 32768, False): 'via rows, 7 slice(s) of 1293 strings: hrx::ragged_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=21 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
    ('headers4', 8, 8192, 32768, True): 'via rows, 7 slice(s) of 1293 strings: hrx::ragged_slice_kernel + hrx::witness_pmd_kernel<4, true, true, false> grid=21 waves=6 ring=4 lds=93888 + hrx::spans_from_masked_pm_kernel',
}
