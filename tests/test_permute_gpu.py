"""LOOKUP PERMUTE on the device (hrx_lookup_permute_device, lookup_permute_kernel of csrc/hrx_kernel_permute.hip).  The yardsticks are the host twin
(hrx_lookup_permute_host over the same counts and table copied to the host), word for word and limb for limb, and hra.permuted_lookup_columns — the numpy
construction — on a sample of strings; neither is the kernel under test.

  regex1               counts from the device counts call on device witness rows at M = 19; 1 and 3 strings (the positions cut into workgroup ranges), the
                       batch at which a lookup becomes one workgroup, minus and plus 1; n_rows = T, T + 1 and around every tile border up to 4097; pitch 4096
  hand-made counts     all zero, every row once, one row holding everything, a full lookup without row 0, one too many, two words of 0xffffffff — overflowing
                       lookups beside sound ones in one call
  defs                 regex2 + regex3, five and eight defs
  tables over a chunk  the synthetic 256-state DFA, 65537 transition rows (22 chunks, the fill list in the workspace): one bin holding nearly all, uniform counts
  modes                indices only, cells only, both; one table run for the call and one per string with distinct challenges
  contract             capture and replay with the call the first of a fresh context, a side stream, a workspace one byte short, refused calls, a host-only context

Every output lies between two poisoned 4-KiB guards and the pitch tails stay poisoned.  No test provokes a fault."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import halo2_regex_amd as hra
from halo2_regex_amd import synth
from test_compress_gpu import thetas_for, on_device
from test_lookup_gpu import batch, device_counts
from test_match_cpu import CFG_H4, CFG_23
from test_permute_cpu import check_against_numpy, hand_made_counts, lookups_of, t_max
from test_verify_gpu import Rows, defs_of_files, CFG_1

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
POISON32, POISON64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
GUARD = 4096                  # bytes before and behind


def guarded(n, dtype):
    """a tensor of n elements of poison between two poisoned guards"""
    size, poison = (4, POISON32) if dtype == torch.int32 else (8, POISON64)
    g = GUARD // size
    raw = torch.full((g + n + g,), poison, dtype=dtype, device=DEV)
    return raw, raw[g:g + n]


def intact(raw, n, dtype):
    size, poison = (4, POISON32) if dtype == torch.int32 else (8, POISON64)
    g = GUARD // size
    return bool((raw[:g] == poison).all()) and bool((raw[g + n:] == poison).all())


class Out:
    """the guarded outputs of one call"""

    def __init__(self, cfg, b_count, n_rows, pitch, idx, cells):
        self.p = pitch if pitch else (n_rows + 3) & ~3
        self.n_rows, self.b_count, self.ncols = n_rows, b_count, 3 * cfg.num_defs
        n = self.ncols * b_count * self.p
        self.bufs = {}
        if idx:
            self.bufs["a_idx"], self.bufs["s_idx"] = guarded(n, torch.int32), guarded(n, torch.int32)
        if cells:
            self.bufs["a_cells"], self.bufs["s_cells"] = guarded(4 * n, torch.int64), guarded(4 * n, torch.int64)
        self.bufs["overflow"] = guarded(b_count, torch.int32)

    def tensors(self):
        return {k: v[1] for k, v in self.bufs.items()}

    def poison(self):
        for k, (raw, t) in self.bufs.items():
            raw.fill_(POISON64 if "cells" in k else POISON32)

    def untouched(self):
        return all(bool((raw == (POISON64 if "cells" in k else POISON32)).all()) for k, (raw, t) in self.bufs.items())

    def numpy(self):
        """the outputs as unsigned arrays in their shapes; the guards and the pitch tails checked"""
        res = {}
        for k, (raw, t) in self.bufs.items():
            assert intact(raw, t.numel(), t.dtype), k + ": a guard was written"
            a = t.cpu().numpy()
            if k == "overflow":
                res[k] = a.view(np.uint32)
            elif "idx" in k:
                res[k] = a.view(np.uint32).reshape(self.ncols, self.b_count, self.p)
                assert (res[k][:, :, self.n_rows:] == POISON32).all(), k + ": a pitch tail was written"
            else:
                res[k] = a.view(np.uint64).reshape(self.ncols, self.b_count, self.p, 4)
                assert (res[k][:, :, self.n_rows:] == POISON64).all(), k + ": a pitch tail was written"
        return res


def device_permute(cfg, d_counts, n_rows, d_table=None, pitch=0, idx=True, stream=None):
    out = Out(cfg, d_counts.shape[0], n_rows, pitch, idx, d_table is not None)
    res = cfg.lookup_permute(d_counts, n_rows, table=d_table, pitch=pitch, out=out.tensors(), stream=stream)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    assert set(res) == set(out.bufs)
    return out.numpy()


def same_as_host(cfg, counts, n_rows, table=None, pitch=0, idx=True, sample=()):
    """counts: uint32 (b_count, W) host array; table: uint64 host array (W, 4) or (b_count, W, 4) or None.  The device outputs against the host twin's; the index
    columns of the strings in `sample` against permuted_lookup_columns"""
    d_counts = torch.from_numpy(counts.view(np.int32)).to(DEV)
    d_table = None if table is None else on_device(table)
    got = device_permute(cfg, d_counts, n_rows, d_table, pitch, idx)
    want = cfg.lookup_permute_host(counts, n_rows, table=table, pitch=pitch, out=("idx", "cells") if idx else ("cells",))
    assert set(got) == set(want)
    for k in want:
        g, w = (got[k], want[k]) if k == "overflow" else (got[k][:, :, :n_rows], want[k][:, :, :n_rows])
        bad = np.argwhere(g != w)
        assert not len(bad), "%s differs from the host twin at %s: n_rows %d, %d strings" % (k, bad[0], n_rows, len(counts))
    if idx and len(sample):
        check_against_numpy(cfg, counts, n_rows, got, sample)
    return got


def host_table(cfg, n_runs, canonical=False):
    th, vals = thetas_for(max(n_runs, 4), seed=8)
    return cfg.lookup_compress_table_host(th[:n_runs] if n_runs else th[3], canonical=canonical).reshape((n_runs, -1, 4) if n_runs else (-1, 4))


def real_counts(cfg, B, M, seed=3):
    chars, lens = batch(B, M, seed=seed)
    got, gm = device_counts(Rows(cfg, "pm-in", chars, lens))
    return got


# ---- regex1 -------------------------------------------------------------------------------------------------------------------------------------
def test_regex1_rows_around_every_tile_border():
    M = 19
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_1), device=0)
    T = t_max(cfg)
    plan = cfg.lookup_permute_plan(1, T)
    tile = plan["tile_rows"]
    assert T == 2843 and T <= plan["chunk_rows"] and cfg.lookup_permute_workspace_bytes(3, T) == 0
    edges = sorted({T, T + 1} | {k * tile + s for k in range(T // tile + 1, 4097 // tile + 1) for s in (-1, 0, 1)})
    assert edges[-1] == 4097
    for B in (1, 3):
        counts = real_counts(cfg, B, M, seed=B)
        table = host_table(cfg, B)
        for n_rows in edges:
            p = cfg.lookup_permute_plan(B, n_rows)
            assert p["groups"] == -(-n_rows // tile) and p["group_rows"] == tile        # few strings: every tile a workgroup of its own
            same_as_host(cfg, counts, n_rows, table, sample=range(B))
    counts = real_counts(cfg, 3, M)
    got = same_as_host(cfg, counts, 4090, host_table(cfg, 0), pitch=4096, sample=[0, 2])
    assert got["a_idx"].shape == (3, 3, 4096) and not got["overflow"].any()


def test_regex1_around_the_batch_that_makes_a_lookup_one_workgroup():
    M = 19
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_1), device=0)
    n_rows = t_max(cfg) + 1
    groups = lambda B: cfg.lookup_permute_plan(B, n_rows)["groups"]
    Bt = next(B for B in range(1, 1 << 12) if groups(B) == 1)
    assert Bt > 2 and groups(Bt - 1) == 2 and cfg.lookup_permute_plan(Bt - 1, n_rows)["group_rows"] == 2048 and groups(1) == 3
    for B in (Bt - 1, Bt + 1):
        counts = real_counts(cfg, B, M, seed=B)
        same_as_host(cfg, counts, n_rows, sample=[0, 1, B - 1])
    counts = real_counts(cfg, 43, M)            # with cells: a range of two tiles and one of one
    assert groups(172) == 2
    same_as_host(cfg, np.tile(counts, (4, 1)), n_rows, host_table(cfg, 0), sample=[7])


@pytest.mark.parametrize("exact", [True, False])
def test_hand_made_counts_and_overflow_beside_sound_lookups(exact):
    cfg = hra.RegexVerifyConfig.configure(8, defs_of_files(CFG_1), device=0)
    n_rows = t_max(cfg) + (0 if exact else 1300)
    names, counts, want_over = hand_made_counts(cfg, n_rows)
    assert want_over.any() and not want_over.all()
    for table in (host_table(cfg, len(counts)), None):
        got = same_as_host(cfg, counts, n_rows, table, sample=range(len(counts)))
        assert np.array_equal(got["overflow"], want_over), names
        col = int(np.log2(want_over.max()))
        for i in np.nonzero(want_over)[0]:
            assert (got["a_idx"][col, i, :n_rows] == 0xffffffff).all() and (got["s_idx"][col, i, :n_rows] == 0xffffffff).all()
            assert table is None or (not got["a_cells"][col, i, :n_rows].any() and not got["s_cells"][col, i, :n_rows].any())


# ---- other def sets -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,names", [("regex23", CFG_23), ("five", CFG_H4 + CFG_23[:1]), ("eight", CFG_H4 * 2)])
def test_other_def_sets(name, names):
    M = 19
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(names), device=0)
    counts = real_counts(cfg, 2, M)
    T = t_max(cfg)
    for n_rows in (max(T, M), max(T, M) + 1, 1024 * (T // 1024 + 1) + 1):
        same_as_host(cfg, counts, n_rows, host_table(cfg, 2), sample=[0, 1])
    hand = hand_made_counts(cfg, T + 5)[1]
    same_as_host(cfg, hand, T + 5, host_table(cfg, 0), sample=range(len(hand)))


# ---- a table of many chunks ---------------------------------------------------------------------------------------------------------------------
def test_the_synthetic_256_state_dfa():
    """65537 transition rows: 22 chunks of the table, the fill list in the workspace, one workgroup per lookup"""
    a_txt, sub_txt = synth.random_dfa(256, seed=2, alphabet=np.arange(256, dtype=np.uint8), n_substr_pairs=200)
    M = 4096
    cfg = hra.RegexVerifyConfig.configure(M, [hra.RegexDefs(hra.AllstrRegexDef(a_txt), [hra.SubstrRegexDef(sub_txt)])], device=0)
    T, W = t_max(cfg), cfg.lookup_words()
    plan = cfg.lookup_permute_plan(2, T)
    assert T == 65537 and plan["groups"] == 1 and T > 21 * plan["chunk_rows"] and cfg.lookup_permute_workspace_bytes(2, T) == 2 * W * 4
    chars = np.full((2, M), ord("x"), np.uint8)
    counts = device_counts(Rows(cfg, "pm-in", chars, np.array([M, M - 3], np.uint32)))[0]
    sl = cfg.lookup_layout()[0]["trans"]
    assert np.count_nonzero(counts[0][sl]) < 300 and counts[0][sl].sum() == M - 1      # a walk round one cycle of the DFA: few bins hold all
    heavy = np.zeros((2, W), np.uint32)
    heavy[0, sl.start + 40000], heavy[0, sl.start + 7] = T - 5, 3      # one bin holds nearly all
    heavy[1, sl.stop - 1] = T                           # the last row holds everything: every other row is in the fill list
    uniform = np.zeros((2, W), np.uint32)
    uniform[0, sl.start:sl.stop:2] = 2                  # every other row twice: sum 65538 <= 65600 only
    uniform[1, sl.start + 1:sl.stop] = 1                # every row but row 0 once
    uniform[:, sl.stop + 1] = 3
    for n_rows in (T, 65600):
        same_as_host(cfg, counts, n_rows, host_table(cfg, 2), sample=[0, 1])
        got = same_as_host(cfg, uniform, n_rows, host_table(cfg, 0), sample=[0, 1])
        assert got["overflow"].tolist() == ([1, 0] if n_rows == T else [0, 0])
        assert not same_as_host(cfg, heavy, n_rows, sample=[0, 1])["overflow"].any()
    # a workspace one byte short, a misaligned one, none
    d_counts = torch.from_numpy(counts.view(np.int32)).to(DEV)
    out = Out(cfg, 2, T, 0, True, False)
    need = cfg.lookup_permute_workspace_bytes(2, T)
    ws = torch.empty(need + 256, dtype=torch.int8, device=DEV)
    for bad in (ws[:need - 1], ws[1:need + 1], None):
        rc = hra.lib.hrx_lookup_permute_device(cfg._ctx, d_counts.data_ptr(), 2, T, 0, out.tensors()["a_idx"].data_ptr(), out.tensors()["s_idx"].data_ptr(), None, 0, None,
                                               None, None, bad.data_ptr() if bad is not None else None, bad.numel() if bad is not None else 0, None)
        assert rc == hra.HRX_ERR_ARG
    torch.cuda.synchronize()
    assert out.untouched()


# ---- modes --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [False, True])
def test_modes_and_table_runs(canonical):
    M = 19
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_23), device=0)
    B = 5
    counts = real_counts(cfg, B, M)
    n_rows = max(t_max(cfg), M) + 2
    per_string, one = host_table(cfg, B, canonical), host_table(cfg, 0, canonical)
    assert not np.array_equal(per_string[0], per_string[1])
    both = same_as_host(cfg, counts, n_rows, per_string, sample=range(B))
    for b in range(B):              # the run of the string, not another's
        assert np.array_equal(both["a_cells"][:, b, :n_rows], per_string[b][both["a_idx"][:, b, :n_rows]])
        assert np.array_equal(both["s_cells"][:, b, :n_rows], per_string[b][both["s_idx"][:, b, :n_rows]])
    shared = same_as_host(cfg, counts, n_rows, one)
    assert np.array_equal(shared["a_cells"][:, :, :n_rows], one[shared["a_idx"][:, :, :n_rows]])
    only_idx = same_as_host(cfg, counts, n_rows)
    only_cells = same_as_host(cfg, counts, n_rows, per_string, idx=False)
    assert set(only_idx) == {"a_idx", "s_idx", "overflow"} and set(only_cells) == {"a_cells", "s_cells", "overflow"}
    assert np.array_equal(only_idx["s_idx"], both["s_idx"]) and np.array_equal(only_cells["s_cells"], both["s_cells"])


# ---- the contract -------------------------------------------------------------------------------------------------------------------------------
def test_capture_replay_as_the_first_call_of_a_fresh_context_and_a_side_stream():
    M = 19
    src = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_1), device=0)
    counts = real_counts(src, 3, M)
    table = host_table(src, 3)
    n_rows = t_max(src) + 1
    want = src.lookup_permute_host(counts, n_rows, table=table)
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_1), device=0)           # no call of any kind on it before the capture
    d_counts, d_table = torch.from_numpy(counts.view(np.int32)).to(DEV), on_device(table)
    out = Out(cfg, 3, n_rows, 0, True, True)
    side = torch.cuda.Stream(DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        cfg.lookup_permute(d_counts, n_rows, table=d_table, out=out.tensors(), stream=side)
    torch.cuda.synchronize()
    assert out.untouched()                      # captured, not run
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        got = out.numpy()
        for k in want:
            assert np.array_equal(got[k] if k == "overflow" else got[k][:, :, :n_rows], want[k] if k == "overflow" else want[k][:, :, :n_rows]), k
        out.poison()
    got = device_permute(cfg, d_counts, n_rows, d_table, stream=side)       # eager, on the side stream
    assert np.array_equal(got["s_cells"][:, :, :n_rows], want["s_cells"][:, :, :n_rows])


def test_the_chain_of_stages_on_two_contexts_used_alternately():
    """witness_batch -> lookup_counts -> lookup_compress_table -> lookup_permute on two device contexts alive at once (one def, two defs), stage by stage in
    turn on the current stream: every stage reads the run's one layout (csrc/hrx_lookup_run.hpp), every output word is the host form's on the same rows"""
    M, B = 16, 3
    cfgs = [hra.RegexVerifyConfig.configure(M, defs_of_files(names), device=0) for names in (CFG_1, CFG_23)]
    chars, lens = batch(B, M, seed=5)
    d_chars, d_lens = torch.from_numpy(chars).to(DEV), torch.from_numpy(lens.astype(np.int32)).to(DEV)
    theta = thetas_for(8, seed=8)[0][7]
    d_theta = on_device(theta)
    rows, d_counts, d_table, res = {}, {}, {}, {}
    for step in range(4):
        for i, cfg in enumerate(cfgs):
            if step == 0:
                rows[i] = cfg.witness_batch(d_chars, d_lens)
            elif step == 1:
                d_counts[i] = cfg.lookup_counts(d_chars, d_lens, rows[i][0])
            elif step == 2:
                d_table[i] = cfg.lookup_compress_table(d_theta)
            else:
                res[i] = cfg.lookup_permute(d_counts[i][0], t_max(cfg) + 1, table=d_table[i][0])
    torch.cuda.synchronize()
    for i, cfg in enumerate(cfgs):
        W, n_rows = cfg.lookup_words(), t_max(cfg) + 1
        rec = rows[i][0].cpu().numpy().view(np.uint32)
        counts, misses = cfg.lookup_counts_host(chars, lens, rec)
        assert np.array_equal(d_counts[i][0].cpu().numpy().view(np.uint32), counts) and np.array_equal(d_counts[i][1].cpu().numpy().view(np.uint32), misses)
        table = cfg.lookup_compress_table_host(theta)
        assert table.shape == (1, W, 4) and np.array_equal(d_table[i].cpu().numpy().view(np.uint64), table)
        want = cfg.lookup_permute_host(counts, n_rows, table=table[0])
        assert set(res[i]) == set(want) == {"a_idx", "s_idx", "a_cells", "s_cells", "overflow"}
        for k in want:
            got = res[i][k].cpu().numpy().view(want[k].dtype)
            assert np.array_equal(got if k == "overflow" else got[:, :, :n_rows], want[k] if k == "overflow" else want[k][:, :, :n_rows]), (i, k)
        assert not want["overflow"].any()


def test_refused_calls_write_nothing_and_a_host_only_context():
    M = 19
    cfg = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_23), device=0)
    B, W, T = 2, cfg.lookup_words(), t_max(cfg)
    n_rows = max(T, M) + 2
    pitch = (n_rows + 3) & ~3
    d_counts = torch.zeros((B, W), dtype=torch.int32, device=DEV)
    d_table = torch.zeros((W, 4), dtype=torch.int64, device=DEV)
    out = Out(cfg, B, n_rows, pitch, True, True)
    t = out.tensors()
    good = dict(counts=d_counts.data_ptr(), b_count=B, n_rows=n_rows, pitch=pitch, a_idx=t["a_idx"].data_ptr(), s_idx=t["s_idx"].data_ptr(), table=d_table.data_ptr(),
                stride=0, a_cells=t["a_cells"].data_ptr(), s_cells=t["s_cells"].data_ptr(), ov=t["overflow"].data_ptr())
    order = ("counts", "b_count", "n_rows", "pitch", "a_idx", "s_idx", "table", "stride", "a_cells", "s_cells", "ov")

    def call(ctx=cfg._ctx, **kw):
        a = dict(good, **kw)
        return hra.lib.hrx_lookup_permute_device(ctx, *[a[k] for k in order], None, 0, None)

    bad = [dict(n_rows=T - 1, pitch=0), dict(n_rows=(1 << 24) + 1, pitch=0), dict(pitch=pitch + 2), dict(pitch=pitch - 4), dict(stride=4), dict(s_idx=None),
           dict(table=None), dict(a_cells=None), dict(a_idx=None, s_idx=None, table=None, a_cells=None, s_cells=None), dict(counts=None),
           dict(counts=good["counts"] + 4), dict(a_idx=good["a_idx"] + 4), dict(s_cells=good["s_cells"] + 8), dict(ov=good["ov"] + 2)]
    for kw in bad:
        assert call(**kw) == hra.HRX_ERR_ARG, kw
    assert call(ctx=None) == hra.HRX_ERR_ARG
    host_only = hra.RegexVerifyConfig.configure(M, defs_of_files(CFG_23), device=hra.HRX_DEVICE_NONE)
    assert call(ctx=host_only._ctx) == hra.HRX_ERR_HIP
    torch.cuda.synchronize()
    assert out.untouched()
    assert call(b_count=0) == hra.HRX_OK and call() == hra.HRX_OK
    torch.cuda.synchronize()
    got = out.numpy()
    assert (got["a_idx"][:, :, :n_rows] != POISON32).all() and not got["overflow"].any()
