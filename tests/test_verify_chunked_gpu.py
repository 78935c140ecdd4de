"""CHUNKED VERIFY on the device (hrx_verify_rows_chunked_device / _planes: verify_chunk_kernel<DT, T, REC> and verify_stitch_kernel of
csrc/hrx_kernel_verify.hip).  The rows come from the device witness entry points; the yardstick is always the UNCHUNKED host word (hrx_verify_rows_host over
the same rows copied to the host) and the torch checker's bits (tests/mock_prover.py) — never the chunked code.  The verdicts and the workspace each lie
between two poisoned 4-KiB guards.

  clean rows, every form     the seven def sets of tests/test_verify_gpu.py at M = 264 x every form x chunk_rows 32 (nine chunks, the last of 8 rows), 64 and 0
  tamper                     the catalogue of tests/verify_cases.py for one, three, five and eight defs (M = 139) in three forms, unjudged cells poisoned first;
                             one-cell changes at rows 95 .. 97 and 127 .. 129
  long ranges                lever definitions, 2048 rows: a range of M - 2 rows whose pending rows wait across up to 63 summaries, ranges taken back three ways,
                             ranges opened and resolved on either side of a chunk border
  block border               65536 + 300 strings x 70 rows, three chunks: a masked cell and a record of a string of the second block, in chunks 1 and 2
  lengths                    n = 0, 31, 32, 33, M; lens > M
  contract                   capture and replay, the first call inside a capture, every refusal, a workspace of exactly the stated size, a host-only context"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import carry_defs as cd
import fr_cases as fc
import halo2_regex_amd as hra
import verify_cases as vc
from mock_prover import FAIL_ACCEPT, FAIL_MASK
from test_verify_cases_cpu import expected
from test_verify_chunked_cpu import apply_far, far_row_batch
from test_verify_gpu import DEV, PM_IN, POISON, SETS, Rows, defs_of_files, defs_of_text, guarded, guards_intact, lever_batch, stress_batches, torch_bits, CFG_A

pytestmark = pytest.mark.gpu
WS_GUARD = 4096
WS_POISON = 0x5A


def guarded_workspace(nbytes):
    raw = torch.full((WS_GUARD + nbytes + WS_GUARD,), WS_POISON, dtype=torch.uint8, device=DEV)
    return raw, raw[WS_GUARD:WS_GUARD + nbytes]


def workspace_guards_intact(raw, nbytes):
    return bool((raw[:WS_GUARD] == WS_POISON).all()) and bool((raw[WS_GUARD + nbytes:] == WS_POISON).all())


def chunked(rows, chunk_rows, lens=None):
    """the chunked device verdicts as uint64: verdicts and a workspace of exactly the stated size between their guards"""
    raw, v = guarded(rows.B)
    need = hra.verify_chunked_workspace_bytes(rows.B, rows.M, chunk_rows if chunk_rows else rows.cfg.verify_chunk_rows(rows.B))
    assert need > 0 and need % (32 * rows.B) == 0
    ws_raw, ws = guarded_workspace(need)
    got = rows.cfg.verify_rows(rows.src, rows.d_lens if lens is None else lens, rows.rec, rows.msk, layout=rows.layout, planes=rows.planes, out=v, chunk_rows=chunk_rows,
                               workspace=ws, **rows.kw)
    torch.cuda.synchronize()
    assert got.data_ptr() == v.data_ptr() and guards_intact(raw, rows.B), "%s chunk_rows %d: a guard of the verdicts was written" % (rows.form, chunk_rows)
    assert workspace_guards_intact(ws_raw, need), "%s chunk_rows %d: a guard of the workspace was written" % (rows.form, chunk_rows)
    return v.cpu().numpy().view(np.uint64)


def same_words(got, want, what):
    bad = np.nonzero(got != want)[0]
    assert not len(bad), "%s: string %d: %s, unchunked host word %s (%d strings differ)" % (what, bad[0], hra.explain_verdict(got[bad[0]]), hra.explain_verdict(want[bad[0]]), len(bad))


@pytest.mark.parametrize("name", list(SETS))
def test_clean_rows_every_form(name):
    M = 264
    make, forms = SETS[name]
    cfg = hra.RegexVerifyConfig.configure(M, make(), device=0)
    assert cfg.verify_chunk_rows(300) >= M          # chunk_rows = 0 is one chunk at this size
    for chars, lens in stress_batches(M):
        for form in forms:
            rows = Rows(cfg, form, chars, lens)
            rec, msk = rows.host_rows()
            want = cfg.verify_rows_host(chars, lens, rec, msk)
            bits = torch_bits(cfg, rows, rec, msk)
            assert np.array_equal((want & np.uint64(0xffffffff)).astype(np.int64), bits)
            for chunk_rows in (32, 64, 0):
                got = chunked(rows, chunk_rows)
                same_words(got, want, "%s %s chunk_rows %d" % (name, form, chunk_rows))
                assert np.array_equal((got & np.uint64(0xffffffff)).astype(np.int64), bits)


@pytest.mark.parametrize("form", ["sm", "pm-in", "planes"])
@pytest.mark.parametrize("name", ["one", "three", "five", "eight"])
def test_tamper(name, form):
    e = expected(name)
    cat = e.cat
    cfg = hra.RegexVerifyConfig.configure(cat.M, defs_of_text(cat.defs_t), device=0)
    rows = Rows(cfg, form, cat.chars, cat.lens)
    rows.poison_unjudged(vc.POISON_REC, vc.POISON_MSK, vc.POISON_CHAR)
    for chunk_rows in (32, 64):
        same_words(chunked(rows, chunk_rows), e.clean, "%s %s clean, poisoned, chunk_rows %d" % (name, form, chunk_rows))
    rows.apply(cat)
    rec, msk = rows.host_rows()
    assert np.array_equal(rec, e.rec_mut) and np.array_equal(msk, e.msk_mut)
    for chunk_rows in (32, 64):
        got = chunked(rows, chunk_rows)
        same_words(got, e.want, "%s %s catalogue chunk_rows %d" % (name, form, chunk_rows))
        assert np.array_equal((got & np.uint64(0xffffffff)).astype(np.int64), e.bits)


@pytest.mark.parametrize("form", ["sm", "pm-in", "planes"])
@pytest.mark.parametrize("name", ["one", "three", "five", "eight"])
def test_cells_at_rows_96_and_128(name, form):
    cat, chars, lens, muts = far_row_batch(name)
    cfg = hra.RegexVerifyConfig.configure(cat.M, defs_of_text(cat.defs_t), device=0)
    rows = Rows(cfg, form, chars, lens)
    rec, msk = rows.host_rows()
    rec2, msk2 = apply_far(muts, rec, msk)
    rb = [(b, r, d, vc.OPS[k][1], vc.OPS[k][2]) for b, k, r, d in muts if vc.OPS[k][0] == "rec"]
    mb = [(b, r, d, vc.OPS[k][1], vc.OPS[k][2]) for b, k, r, d in muts if vc.OPS[k][0] == "msk"]
    col = lambda rowsl, i: np.array([m[i] for m in rowsl], np.int64)
    which, idx = rows.rec_cells(col(rb, 0), col(rb, 1), col(rb, 2))
    rows.update(rows.rec_buffers(), which, idx, col(rb, 3), col(rb, 4))
    rows.update([rows.msk_buffer()], np.zeros(len(mb)), rows.msk_cells(col(mb, 0), col(mb, 1)), col(mb, 3), col(mb, 4))
    r3, m3 = rows.host_rows()
    assert np.array_equal(r3, rec2) and np.array_equal(m3, msk2)
    want = cfg.verify_rows_host(chars, lens, rec2, msk2)
    assert (want[1:-1] != 0).all() and want[0] == 0 and want[-1] == 0
    for chunk_rows in (32, 64):
        same_words(chunked(rows, chunk_rows), want, "%s %s chunk_rows %d" % (name, form, chunk_rows))


@pytest.mark.parametrize("D,form", [(1, "pm-in"), (3, "planes")], ids=["one-def-interleaved", "three-defs-planes"])
def test_long_ranges(D, form):
    """tests/test_verify_gpu.py test_long_ranges through 64, 8 and 2 chunks: the pending rows of the confirmed range wait across up to 63 summaries for the end-only event
    (the first backward event of the last chunk); the take-backs filled in as if revealed report at the range's first row, 63 chunks before the event that decides them"""
    M = 2048
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_text(cd.lever_defs(D)), device=0)
    chars, lens, cases = lever_batch(M, D)
    rows = Rows(cfg, form, chars, lens)
    assert (rows.st.cpu().numpy() & 0xff == 0).all()
    rec, msk = rows.host_rows()
    assert (msk[0, :M - 2] != 0).all() and not msk[1:4].any()
    sizes = (32, 256, 1024)
    clean = rows.host_words()
    for b, (kind, a, end) in enumerate(cases):
        assert clean[b] == (FAIL_ACCEPT | int(lens[b]) << 32 if kind == "string_end" else 0), (kind, hra.explain_verdict(clean[b]))
    assert (clean[4:] == 0).all()
    for chunk_rows in sizes:
        same_words(chunked(rows, chunk_rows), clean, "clean chunk_rows %d" % chunk_rows)
    for row in (1, 1000, M - 3):
        keep = rows.get_msk(0, row)
        rows.set_msk(0, row, 0)
        want = rows.host_words()
        assert want[0] == (FAIL_MASK | row << 32) and np.array_equal(want[1:], clean[1:])
        for chunk_rows in sizes:
            same_words(chunked(rows, chunk_rows), want, "row %d blanked, chunk_rows %d" % (row, chunk_rows))
        rows.set_msk(0, row, keep)
    for b in (1, 2, 3):
        kind, a, end = cases[b]
        r = np.arange(a, min(end, int(lens[b])))
        value = chars[b, r].astype(np.int64) | ((rec[b, r] >> 16) & 0xff).sum(axis=1).astype(np.int64) << 8
        rows.update([rows.msk_buffer()], np.zeros(len(r)), rows.msk_cells(np.full(len(r), b), r), np.zeros(len(r)), value)
    want = rows.host_words()
    for b in (1, 2, 3):
        assert int(want[b]) & 0xffffffff == (FAIL_MASK | (int(clean[b]) & 0xffffffff)) and int(want[b]) >> 32 == cases[b][1], (cases[b], hra.explain_verdict(want[b]))
    assert want[0] == 0 and (want[4:] == 0).all()
    for chunk_rows in sizes:
        same_words(chunked(rows, chunk_rows), want, "take-backs filled in, chunk_rows %d" % chunk_rows)


def border_batch(M, D):
    """ranges opened at border - 1, border, border + 1 of a 32-row chunk and confirmed (sc_confirmed) or taken back by a second start (sc_second_start) at
    border - 1, border, border + 1 of a later one: (chars, lens, [(kind, first row, resolving row)])"""
    ko, kr = 0, D - 1
    made = []
    for a in (31, 32, 33):
        for b in (63, 64, 65, 1023, 1024, 1025):
            made.append(("confirmed",) + cd.sc_confirmed(M, a, b, ko, kr))
            made.append(("taken_back",) + cd.sc_second_start(M, a, b, ko, kr))
    B = 64
    assert len(made) <= B
    chars = np.zeros((B, M + 16), np.uint8)
    lens = np.full(B, M, np.uint32)
    chars[:, :M] = cd.LEVERS[0][0]
    cases = []
    for b, (kind, v, code, ranges) in enumerate(made):
        assert code == 0
        chars[b, :] = 0
        chars[b, :len(v)] = v
        lens[b] = len(v)
        cases.append((kind, ranges[0][0], ranges[0][1]))
    return chars, lens, cases


@pytest.mark.parametrize("D,form", [(1, "pm-in"), (3, "planes")], ids=["one-def-interleaved", "three-defs-planes"])
def test_ranges_at_chunk_borders(D, form):
    M = 2048
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_text(cd.lever_defs(D)), device=0)
    chars, lens, cases = border_batch(M, D)
    rows = Rows(cfg, form, chars, lens)
    assert (rows.st.cpu().numpy() & 0xff == 0).all()
    rec, msk = rows.host_rows()
    clean = rows.host_words()
    for b, (kind, a, end) in enumerate(cases):
        assert (msk[b, a:end + 1] != 0).all() if kind == "confirmed" else not msk[b, a:end].any(), (kind, a, end)
    for chunk_rows in (32, 1024):
        same_words(chunked(rows, chunk_rows), clean, "clean chunk_rows %d" % chunk_rows)
    # a confirmed range loses its first and its last cell but one; a range taken back has them filled in as if revealed
    cells = [(b, r) for b, (kind, a, end) in enumerate(cases) for r in (a, end - 1)]
    b_, r_ = np.array([c[0] for c in cells]), np.array([c[1] for c in cells])
    value = np.where(msk[b_, r_] != 0, 0, chars[b_, r_].astype(np.int64) | ((rec[b_, r_] >> 16) & 0xff).sum(axis=1).astype(np.int64) << 8)
    rows.update([rows.msk_buffer()], np.zeros(len(cells)), rows.msk_cells(b_, r_), np.zeros(len(cells)), value)
    want = rows.host_words()
    for b, (kind, a, end) in enumerate(cases):
        assert int(want[b]) & FAIL_MASK and int(want[b]) >> 32 <= a, (cases[b], hra.explain_verdict(want[b]))
    assert np.array_equal(want[len(cases):], clean[len(cases):])
    for chunk_rows in (32, 1024):
        same_words(chunked(rows, chunk_rows), want, "changed chunk_rows %d" % chunk_rows)


@pytest.mark.parametrize("form", ["pm", "pm-in"])
def test_block_border(form):
    """65536 + 300 strings x 70 rows, chunk_rows = 32 (three chunks, the last of 6 rows): the second block's string count enters every index of its chunks.  Clean; then one
    masked cell of chunk 1 and one record of chunk 2 of string 65536 + 5 changed on the device: exactly that string, with the unchunked host word"""
    chars, lens = tall_batch_70()
    B, M = len(lens), 70
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_text([fc.sweep_def(fc.BIG_SWEEP_L)]), device=0)
    rows = Rows(cfg, form, chars, lens)
    clean = rows.host_words()
    same_words(chunked(rows, 32), clean, "clean")
    b = 65536 + 5
    rows.set_msk(b, 40, rows.get_msk(b, 40) ^ 0x0101)
    rows.xor_rec(b, 66, 0, 1)
    want = rows.host_words()
    got = chunked(rows, 32)
    same_words(got, want, "changed")
    assert np.nonzero(got != clean)[0].tolist() == [b] and int(got[b]) & FAIL_MASK and int(got[b]) & (hra.VERIFY_TRANSITION | hra.VERIFY_PADDING), hra.explain_verdict(got[b])


def tall_batch_70():
    """fr_cases.tall_batch's strings (65536 + 300 of them, up to 19 bytes) in rows of 80 input bytes: M = 70"""
    chars, lens = fc.tall_batch()
    wide = np.zeros((len(lens), 80), np.uint8)
    wide[:, :chars.shape[1]] = chars
    return wide, lens


def test_lengths():
    """n = 0, 31, 32, 33 and M at chunk_rows = 32 (enable drops at, before and behind the border); lens = M + 1 on one string: all ones, every other word unchanged"""
    M, D = 139, 2
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_text(cd.lever_defs(D)), device=0)
    ns = [0, 31, 32, 33, M]
    B = 70
    lens = np.array([ns[b % 5] for b in range(B)], np.uint32)
    rng = np.random.default_rng(3)
    pool = np.frombuffer(b"".join(cd.LEVERS[:D]), np.uint8)
    chars = np.zeros((B, (M + 15) // 16 * 16 + 16), np.uint8)
    for b in range(B):
        chars[b, :lens[b]] = pool[rng.integers(0, len(pool), size=int(lens[b]))]
    for form in ("sm", "pm-in", "planes"):
        rows = Rows(cfg, form, chars, lens)
        clean = rows.host_words()
        got = chunked(rows, 32)
        same_words(got, clean, form)
        # the state of row n and the masked cell of row n - 1 / 0 of every string
        b = np.arange(B)
        which, idx = rows.rec_cells(b, np.minimum(lens, M - 1), b % D)
        rows.update(rows.rec_buffers(), which, idx, np.full(B, 0xffffffff), np.ones(B))
        rows.update([rows.msk_buffer()], np.zeros(B), rows.msk_cells(b, np.maximum(lens.astype(np.int64) - 1, 0)), np.full(B, 0xffff), np.full(B, 0x0101))
        want = rows.host_words()
        assert (want != 0).all()
        same_words(chunked(rows, 32), want, form + " changed")
        too_long = rows.lens.copy()
        too_long[33] = M + 1
        got = chunked(rows, 32, lens=torch.from_numpy(too_long.astype(np.int32)).to(DEV))
        assert got[33] == np.uint64(0xffffffffffffffff) and np.array_equal(np.delete(got, 33), np.delete(want, 33))
        same_words(got, rows.host_words(lens=too_long), form + " lens > M")


# ---- contract ----------------------------------------------------------------------------------------------------------------------------------------
def small_rows(cfg_of=None, form="pm-in", M=139, B=70):
    from halo2_regex_amd import synth
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_A), device=0) if cfg_of is None else cfg_of
    chars, lens = synth.ragged(B, M, seed=3)
    return Rows(cfg, form, np.ascontiguousarray(chars), lens)


def test_capture_and_replay():
    """a fresh context inside a capture: HRX_ERR_STATE and nothing written; after one eager call the two launches capture, and replay twice with the same verdicts"""
    rows = small_rows()
    raw, v = guarded(rows.B)
    need = hra.verify_chunked_workspace_bytes(rows.B, rows.M, 32)
    ws_raw, ws = guarded_workspace(need)
    call = lambda stream: rows.cfg.verify_rows(rows.src, rows.d_lens, rows.rec, rows.msk, layout=rows.layout, out=v, stream=stream, chunk_rows=32, workspace=ws, **rows.kw)
    side = torch.cuda.Stream(DEV)
    dummy = torch.zeros(16, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):                 # no verify call before this one
        dummy.add_(1)
        with pytest.raises(hra.HrxError) as e:
            call(side)
    assert e.value.code == hra.HRX_ERR_STATE
    g.replay()
    torch.cuda.synchronize()
    assert bool((raw == POISON).all()) and bool((ws_raw == WS_POISON).all())
    want = rows.host_words()
    same_words(chunked(rows, 32), want, "eager")           # the eager call: builds and uploads the tables
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=side):
        call(side)
    torch.cuda.synchronize()
    assert bool((raw == POISON).all()) and bool((ws_raw == WS_POISON).all())        # captured, not run
    for _ in range(2):
        g2.replay()
        torch.cuda.synchronize()
        assert np.array_equal(v.cpu().numpy().view(np.uint64), want) and guards_intact(raw, rows.B) and workspace_guards_intact(ws_raw, need)
        v.fill_(POISON)


def test_refused_calls_write_nothing():
    rows = small_rows(form="planes-in")
    cfg, B, M = rows.cfg, rows.B, rows.M
    raw, v = guarded(B)
    need = hra.verify_chunked_workspace_bytes(B, M, 32)
    assert need == 32 * 5 * B
    ws_raw, ws = guarded_workspace(need)
    lib, ctx = hra.lib, cfg._ctx
    arr = (C.c_void_p * 2)(*[p.data_ptr() for p in rows.planes])
    common = (rows.src.data_ptr(), rows.stride, rows.d_lens.data_ptr())
    planes = lambda chunk_rows, wsp, wsb, vp=None, layout=PM_IN, n=2, a=arr, m=M: lib.hrx_verify_rows_chunked_device_planes(
        ctx, layout, *common, a, n, rows.msk.data_ptr(), B, m, chunk_rows, wsp, wsb, v.data_ptr() if vp is None else vp, None)
    want = rows.host_words()
    assert planes(32, ws.data_ptr(), need) == hra.HRX_OK               # a workspace of exactly the stated size
    torch.cuda.synchronize()
    assert np.array_equal(v.cpu().numpy().view(np.uint64), want) and guards_intact(raw, B) and workspace_guards_intact(ws_raw, need)
    v.fill_(POISON)
    ws.fill_(WS_POISON)
    for bad in (1, 31, 33, 48, 100):
        assert planes(bad, ws.data_ptr(), need) == hra.HRX_ERR_ARG                      # no multiple of 32
    assert planes(32, None, need) == hra.HRX_ERR_ARG                                    # NULL workspace
    assert planes(32, ws.data_ptr() + 4, need) == hra.HRX_ERR_ARG                       # misaligned
    assert planes(32, ws.data_ptr(), need - 1) == hra.HRX_ERR_ARG                       # too small
    assert planes(32, ws.data_ptr(), 0) == hra.HRX_ERR_ARG
    assert planes(64, ws.data_ptr(), hra.verify_chunked_workspace_bytes(B, M, 64) - 32) == hra.HRX_ERR_ARG
    # whatever the unchunked call refuses
    assert planes(32, ws.data_ptr(), need, vp=v.data_ptr() + 4) == hra.HRX_ERR_ARG
    assert planes(32, ws.data_ptr(), need, layout=hra.LAYOUT_STRING_MAJOR) == hra.HRX_ERR_ARG
    assert planes(32, ws.data_ptr(), need, n=1) == hra.HRX_ERR_ARG and planes(32, ws.data_ptr(), need, n=3) == hra.HRX_ERR_ARG
    null = (C.c_void_p * 2)(rows.planes[0].data_ptr(), None)
    assert planes(32, ws.data_ptr(), need, a=null) == hra.HRX_ERR_ARG and planes(32, ws.data_ptr(), need, a=None) == hra.HRX_ERR_ARG
    assert planes(32, ws.data_ptr(), 1 << 40, m=(1 << 24) + 1) == hra.HRX_ERR_ARG
    sm = small_rows(cfg_of=cfg, form="sm")
    args = (sm.src.data_ptr(), sm.stride, sm.d_lens.data_ptr(), sm.rec.data_ptr())
    tail = (B, M, 32, ws.data_ptr(), need, v.data_ptr(), None)
    assert lib.hrx_verify_rows_chunked_device(ctx, 0, *args, M - 1, sm.msk.data_ptr(), 0, *tail) == hra.HRX_ERR_ARG          # pitch < M
    assert lib.hrx_verify_rows_chunked_device(ctx, 4, *args, 0, sm.msk.data_ptr(), 0, *tail) == hra.HRX_ERR_ARG
    assert lib.hrx_verify_rows_chunked_device(ctx, 0, *args, 0, None, 0, *tail) == hra.HRX_ERR_ARG
    assert lib.hrx_verify_rows_chunked_device(None, 0, *args, 0, sm.msk.data_ptr(), 0, *tail) == hra.HRX_ERR_ARG
    host_only = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_A), device=hra.HRX_DEVICE_NONE)
    assert lib.hrx_verify_rows_chunked_device(host_only._ctx, 0, *args, 0, sm.msk.data_ptr(), 0, *tail) == hra.HRX_ERR_HIP
    assert lib.hrx_verify_rows_chunked_device_planes(host_only._ctx, PM_IN, *common, arr, 2, rows.msk.data_ptr(), B, M, 32, ws.data_ptr(), need, v.data_ptr(), None) == hra.HRX_ERR_HIP
    torch.cuda.synchronize()
    assert bool((raw == POISON).all()) and bool((ws_raw == WS_POISON).all())
    assert lib.hrx_verify_rows_chunked_device(ctx, 0, *args, 0, sm.msk.data_ptr(), 0, *tail) == hra.HRX_OK
    torch.cuda.synchronize()
    assert np.array_equal(v.cpu().numpy().view(np.uint64), sm.host_words()) and guards_intact(raw, B) and workspace_guards_intact(ws_raw, need)
    # the workspace is allocated where the caller passes none, on a clone with tables of its own too
    got = cfg.clone().verify_rows(sm.src, sm.d_lens, sm.rec, sm.msk, chunk_rows=64)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy().view(np.uint64), sm.host_words())
