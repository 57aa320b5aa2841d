"""CPU-side checks: the C-ABI library loads and exports every symbol include/mrmt3_hip.h declares
(no compute calls without a GPU), the frontend oracle's known-answer anchors, and the inference
harness restatement (hand-derived answers from inference.py:64-136,206-215)."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from mrmt3 import lib


def test_library_exports_every_declared_symbol():
    assert os.path.exists(lib.LIB_PATH), "run __graft_entry__.build() first"
    names = lib.header_symbols()
    assert len(names) >= 25
    so = ctypes.CDLL(lib.LIB_PATH)
    missing = [n for n in names if not hasattr(so, n)]
    assert not missing, missing
    assert set(names) == set(lib._SIGS), set(names) ^ set(lib._SIGS)
    assert lib.load().mrmt3_version() >= 100


def test_header_derived_signatures_match_hand_written_ones():
    """lib._SIGS is parsed from the prototypes of include/mrmt3_hip.h: a few signatures typed out by hand here, so that a
    parser regression cannot hide behind itself — the widest argument list, a size_t and a `const char*` return, a
    `void` return, handle out-parameters, `const char*` and 64-bit scalar arguments."""
    vp, ci, cf, cu64, cu32, csz = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint32,
                                   ctypes.c_size_t)
    out_handle = ctypes.POINTER(ctypes.c_void_p)
    want = {
        "mrmt3_attn_bwd_varlen": (ci, [vp, ci, vp, ci, vp, ci, vp, ci, vp, vp, ci, vp, vp, vp, ci, vp, ci, vp, ci, vp, vp, ci, ci,
                                       ci, ci, ci, ci, ci, cf, cu64, vp, cu32, vp]),
        "mrmt3_gemm_tn_workspace_bytes": (csz, [ci, ci, ci]),
        "mrmt3_gemm_tn": (ci, [vp, ci, vp, ci, vp, ci, ci, ci, ci, ci, vp, csz, vp]),
        "mrmt3_last_error": (ctypes.c_char_p, []),
        "mrmt3_version": (ci, []),
        "mrmt3_host_alloc": (vp, [csz]),
        "mrmt3_host_free": (None, [vp]),
        "mrmt3_set_knob": (ci, [ctypes.c_char_p, ci]),
        "mrmt3_decoder_create": (ci, [out_handle, ci, ci, ci, ci, ci, ci, ci, ci, ci, cf]),
        "mrmt3_comm_create": (ci, [vp, ci, ci, out_handle]),
        "mrmt3_stream_create": (ci, [out_handle, ci]),
        "mrmt3_logmel_crops_fwd": (ci, [vp, ctypes.c_longlong, vp, ci, ci, ci, vp, vp, vp, vp, vp, ci, ci, vp, ci, ci, vp, vp]),
        "mrmt3_adamw_step": (ci, [vp, vp, vp, vp, vp, csz, vp, ci, csz, vp, vp, cf, cf, cf, cf, cf, cf, vp, cf, vp, vp]),
    }
    assert len(want["mrmt3_attn_bwd_varlen"][1]) == 33
    for name, sig in want.items():
        assert lib._SIGS[name] == sig, (name, lib._SIGS[name])
    fn = lib.load().mrmt3_attn_bwd_varlen                    # ... and load() has applied them
    assert fn.restype is ci and list(fn.argtypes) == want["mrmt3_attn_bwd_varlen"][1]
    assert lib.load().mrmt3_gemm_tn_workspace_bytes.restype is csz and lib.load().mrmt3_last_error.restype is ctypes.c_char_p
    # a type the parser does not know is an error, not a guess
    with pytest.raises(TypeError):
        lib._ctype("double", "test")
    with pytest.raises(TypeError):
        lib._ctype("mrmt3_tn_gsite", "test")


def test_product_library_carries_no_kernel_diagnostics():
    """the round-4 experiments (knock-out bits, start skews, per-workgroup time stamps) are compiled only
    into the -DMRMT3_DIAG twin that profiles/tools load; the product library neither exports the trace entry point nor
    reads the diagnostic switches, and no launch path calls getenv (knobs: read once, mrmt3_set_knob overrides)."""
    so = ctypes.CDLL(lib.LIB_PATH)
    assert not hasattr(so, "mrmt3_gemm_rows_trace")
    blob = open(lib.LIB_PATH, "rb").read()
    for switch in (b"MRMT3_ROWS_DBG", b"MRMT3_GEMM8_DBG", b"MRMT3_ROWS_SKEW_FINE", b"MRMT3_GEMM8_SKEW", b"MRMT3_GEMM8_GRID"):
        assert switch not in blob, switch
    diag = os.path.join(os.path.dirname(lib.LIB_PATH), "libmrmt3_hip_diag.so")
    assert os.path.exists(diag), "run __graft_entry__.build() first (make -C mr-mt3_amd/csrc diag)"
    dso = ctypes.CDLL(diag)
    assert hasattr(dso, "mrmt3_gemm_rows_trace") and b"MRMT3_ROWS_DBG" in open(diag, "rb").read()
    # the only getenv call sites of the sources: the knob registry (api.hip) and the RCCL path (comm.hip, once per process)
    src = os.path.join(os.path.dirname(os.path.dirname(lib.LIB_PATH)), "csrc")
    users = sorted(f for f in os.listdir(src) if f.endswith((".hip", ".h")) and "getenv(" in open(os.path.join(src, f)).read())
    assert users == ["api.hip", "comm.hip"], users


def test_knobs_are_read_once_and_overridden_through_the_abi(monkeypatch):
    L = lib.load()
    lib.reset_knobs()
    monkeypatch.delenv("MRMT3_ROWS_BM", raising=False)
    assert L.mrmt3_gemm_nt_normbwd_partial_rows(4096) == 64          # 64-row tiles below 32 641 rows
    monkeypatch.setenv("MRMT3_ROWS_BM", "128")                          # the environment is not looked at again ...
    assert L.mrmt3_gemm_nt_normbwd_partial_rows(4096) == 64
    lib.set_knob("MRMT3_ROWS_BM", 128)                                  # ... an override is
    assert L.mrmt3_gemm_nt_normbwd_partial_rows(4096) == 32
    lib.set_knob("MRMT3_ROWS_BM", 64)
    assert L.mrmt3_gemm_nt_normbwd_partial_rows(4096) == 64
    lib.reset_knobs()                                                   # back to the environment (re-read once)
    assert L.mrmt3_gemm_nt_normbwd_partial_rows(4096) == 32
    monkeypatch.delenv("MRMT3_ROWS_BM")
    lib.reset_knobs()
    assert L.mrmt3_gemm_nt_normbwd_partial_rows(4096) == 64
    with pytest.raises(RuntimeError):
        lib.set_knob("NOT_A_KNOB", 1)


def test_device_code_has_no_packed_f32_instructions(tmp_path):
    """The build contract of csrc/Makefile (`SLP_FLAG`): no `v_pk_{add,mul,fma}_f32` / `v_pk_mov_b32` in ANY code object of the
    library.  On gfx950 a packed f32 instruction with a half swap returns a wrong low half in lanes 48-63 while an
    LDS-DMA + MFMA kernel shares the CU (profiles/r04_lds_read_fault.txt) - the cause of the two-rank
    and two-stream mismatches of rounds 2-3.  Also checks that the hot files are really there (MFMA counts)."""
    import shutil
    import subprocess
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("no llvm-objdump in this image")
    so = str(tmp_path / "lib.so")
    shutil.copy(lib.LIB_PATH, so)                      # --offloading extracts next to its input
    subprocess.run([objdump, "--offloading", so], check=True, capture_output=True)
    objs = sorted(str(f) for f in tmp_path.iterdir() if f.name.endswith("gfx950"))
    assert len(objs) >= 10, objs
    packed = re.compile(r"\bv_pk_(add|mul|fma)_f32\b|\bv_pk_mov_b32\b")
    n_mfma = n_dma = 0
    for o in objs:
        asm = subprocess.run([objdump, "-d", o], check=True, capture_output=True, text=True).stdout
        hits = [l.strip() for l in asm.splitlines() if packed.search(l)]
        assert not hits, (os.path.basename(o), hits[:3])
        n_mfma += asm.count("v_mfma_f32_16x16x32_bf16")
        n_dma += len(re.findall(r"buffer_load_dword(x[34])? .* lds", asm)) + asm.count("global_load_lds_dword")
    assert n_mfma > 4000 and n_dma > 400, (n_mfma, n_dma)


def test_comm_entry_points_resolve_rccl_without_linking_it():
    """csrc/comm.hip finds RCCL with dlopen at first use (here: the copy torch has mapped); the library itself must not
    carry a link-time dependency on it.  ncclGetUniqueId needs no device, so the id call works on this CPU box; argument
    errors of the other entry points come back as codes with a message."""
    import subprocess
    so = lib.load()
    needed = subprocess.run(["readelf", "-d", lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "NEEDED" in needed and "rccl" not in needed.lower() and "nccl" not in needed.lower()
    a, b = lib.Comm.unique_id(), lib.Comm.unique_id()
    assert len(a) == len(b) == lib.COMM_ID_BYTES == 128 and a != b
    assert so.mrmt3_comm_unique_id(None) != 0 and b"null" in so.mrmt3_last_error()
    h = ctypes.c_void_p()
    assert so.mrmt3_comm_create(ctypes.create_string_buffer(a, 128), 2, 2, ctypes.byref(h)) != 0     # rank out of range
    assert b"rank 2 of 2" in so.mrmt3_last_error() and not h
    assert so.mrmt3_comm_destroy(None) == 0
    assert so.mrmt3_allreduce(None, None, 0, 0, 0, None) != 0


def test_product_path_refuses_cpu_tensors():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lib.gemm_nt(torch.zeros(128, 64), torch.zeros(128, 64))


def test_filterbank_anchors():
    """SURVEY §8c anchors for the (unpinned) torchaudio filterbank restatement."""
    from oracle import logmel_ref
    from contrib import spectrograms as sp
    fb = logmel_ref.melscale_fbanks()
    assert fb.shape == (1025, 512)
    assert int((fb > 0).sum()) == 1934
    zero_filters = np.nonzero((fb.numpy() > 0).sum(0) == 0)[0]
    assert len(zero_filters) == 2 and zero_filters.max() <= 10
    nzbins = np.nonzero((fb.numpy() > 0).sum(1))[0]
    assert nzbins.min() == 3 and nzbins.max() == 972
    # the product builds the same matrix (same fp32 torch ops)
    assert torch.equal(sp.mel_filterbank(1025, 20.0, 7600.0, 512, 16000), fb)


def test_frontend_oracle_known_answers():
    from oracle import logmel_ref
    x = np.random.RandomState(0).uniform(-1, 1, 32768).astype(np.float32)
    assert logmel_ref.pad_end(torch.from_numpy(x)).shape[-1] == 32768 + 1920
    mel = logmel_ref.compute_spectrogram(x)
    assert mel.shape == (256, 512) and mel.dtype == np.float32
    fb = logmel_ref.melscale_fbanks().numpy()
    dead = np.nonzero((fb > 0).sum(0) == 0)[0]
    assert np.allclose(mel[:, dead], math.log(1e-5))
    assert np.allclose(logmel_ref.normalize_mel(mel)[:, dead], 0.02865, atol=1e-5)
    # pure tone at bin 128 (1 kHz): the loudest mel filter is the one whose triangle covers it
    t = np.arange(32768) / 16000.0
    tone = np.sin(2 * np.pi * 1000.0 * t).astype(np.float32)
    m = logmel_ref.compute_spectrogram(tone)[5]
    assert fb[128, m.argmax()] > 0.5


def test_inference_harness_known_answers():
    from oracle import logmel_ref
    import inference as prod
    for n, nfr, pads in ((40000, 313, [256, 57]), (32768, 257, [256, 1])):
        audio = np.random.RandomState(n).uniform(-1, 1, n).astype(np.float32)
        fr, times = logmel_ref.audio_to_frames(audio)
        assert fr.shape == (nfr, 128)
        segs, ft, paddings = logmel_ref.split_into_segments(fr, times)
        assert segs.shape == (2, 256, 128) and paddings == pads
        # product host logic agrees with the restatement
        pfr, ptimes = prod.audio_to_frames(audio)
        psegs, pft, ppads = prod.split_into_segments(pfr, ptimes)
        assert np.array_equal(psegs, segs) and np.array_equal(pft, ft) and ppads == pads
    ids = np.array([[0, 7, 9, 1, 5]])
    assert logmel_ref.postprocess_batch(ids).tolist() == [[4, 6, -1, -1]]
    assert prod.postprocess_batch(torch.from_numpy(ids)).tolist() == [[4, 6, -1, -1]]


def test_every_binding_the_host_code_calls_exists():
    """A missing Python wrapper only shows up when the GPU path runs: catch it here by scanning the host modules for
    `lib.<name>` uses."""
    import glob
    import os
    import re
    from mrmt3 import lib
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mr-mt3_amd")
    used = set()
    for path in glob.glob(os.path.join(root, "**", "*.py"), recursive=True) + [os.path.join(os.path.dirname(root), "bench.py"),
                                                                                os.path.join(os.path.dirname(root), "__graft_entry__.py")]:
        if path.endswith(os.path.join("mrmt3", "lib.py")):
            continue
        with open(path) as f:
            used |= set(re.findall(r"\blib\.([A-Za-z_][A-Za-z0-9_]*)", f.read()))
    missing = sorted(n for n in used if not hasattr(lib, n))
    assert not missing, missing
    assert {"gemm_nt", "gemm_tn", "attn_fwd", "attn_bwd", "add_rmsnorm_bwd", "embed_bwd", "lmhead_cross_entropy",
            "gemm_nt_geglu", "TnGroup"} <= used


def test_master_version_sees_writes_through_reparented_parameters():
    """After `.to()` / `_apply` every nn.Parameter owns a version counter of its own: writes by
    torch.optim or load_state_dict must still invalidate the bf16 shadows."""
    import torch
    from mrmt3.synthetic import T5_SMALL
    from models.t5 import T5ForConditionalGeneration
    cfg = dict(T5_SMALL, num_layers=1, num_decoder_layers=1)
    m = T5ForConditionalGeneration(cfg)
    m._apply(lambda t: t.clone())                       # what .to(device) does, on the CPU
    v0 = m.flat.master_version()
    assert m.flat.P._version == m.flat.P._version       # P's own counter is not what moves below
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    p_ver = m.flat.P._version
    opt.step()
    assert m.flat.master_version() != v0
    v1 = m.flat.master_version()
    other = {k: v + 1 for k, v in m.state_dict().items()}
    m.load_state_dict(other)
    assert m.flat.master_version() != v1
    assert torch.equal(m.flat.master("lm_head.weight"), other["lm_head.weight"])
    del p_ver


def test_grouped_weight_gradient_plan_covers_every_tile_once():
    """mrmt3_tn_group_plan is host code: for the weight gradients of a decoder + encoder gradient bucket, every
    (gradient, 256 x 256 tile) is covered by token ranges that partition [0, M) in units of 128 rows, each item owns
    its own 256-KiB partial tile inside the scratch buffer, the reduce records name exactly those partial tiles, and
    the busiest workgroup carries at most 15 % more K steps than the average (the planner's whole purpose)."""
    import ctypes as C
    import numpy as np
    from mrmt3 import lib as L
    lib = L.load()
    shapes = [(65536, 512, 1024), (65536, 2048, 512), (65536, 512, 384), (65536, 384, 512), (16384, 768, 512),
              (65536, 1152, 512), (16384, 2048, 512), (16384 + 72, 1152, 512), (4096, 1536, 512)] * 2
    arr = (L._TnGSite * len(shapes))()
    for i, (M, N1, N2) in enumerate(shapes):
        arr[i] = L._TnGSite(0x100000 * (i + 1), 0x200000 * (i + 1), 0x7000000 + 0x100000 * i, N1, N2, N2, M, N1, N2, 1, 0)
    info = L._TnGInfo()
    assert lib.mrmt3_tn_group_plan(arr, len(shapes), None, None, 0, C.byref(info)) == 0
    host = np.zeros(info.table_bytes, np.uint8)
    slab0 = 0x40000000
    assert lib.mrmt3_tn_group_plan(arr, len(shapes), C.c_void_p(slab0), C.c_void_p(host.ctypes.data), host.size, C.byref(info)) == 0
    item_t = np.dtype([("A", "<u8"), ("B", "<u8"), ("out", "<u8"), ("lda", "<i4"), ("ldb", "<i4"), ("ldo", "<i4"),
                       ("M", "<i4"), ("N1", "<i4"), ("N2", "<i4"), ("a0", "<i4"), ("b0", "<i4"), ("rmin", "<i4"),
                       ("cmin", "<i4"), ("row0", "<i4"), ("nk", "<i4"), ("sync_idx", "<i4"), ("sync_n", "<i4")])
    rt_t = np.dtype([("slab", "<u8"), ("C", "<u8"), ("ldc", "<i4"), ("a0", "<i4"), ("b0", "<i4"), ("rmin", "<i4"),
                     ("cmin", "<i4"), ("n_part", "<i4"), ("acc", "<i4"), ("pad", "<i4")])
    assert item_t.itemsize == 80 and rt_t.itemsize == 48
    items = np.frombuffer(host[:info.n_items * 80].tobytes(), dtype=item_t)
    rts = np.frombuffer(host[info.rtile_offset:info.rtile_offset + info.n_rtiles * 48].tobytes(), dtype=rt_t)
    assert info.n_rtiles == sum(-(-n1 // 256) * -(-n2 // 256) for _, n1, n2 in shapes)
    cover, slabs = {}, set()
    for it in items:
        key = (int(it["A"]), int(it["a0"]), int(it["b0"]))
        cover.setdefault(key, []).append((int(it["row0"]), int(it["nk"]) * 64))
        tile_slab = int(it["out"]) + 4 * (int(it["a0"]) * 256 + int(it["b0"]))       # undo the pre-offset
        assert tile_slab >= slab0 and (tile_slab - slab0) % (256 * 1024) == 0 and tile_slab + 256 * 1024 <= slab0 + info.slab_bytes
        assert tile_slab not in slabs
        slabs.add(tile_slab)
        assert it["nk"] % 2 == 0 and it["ldo"] == 256 and it["row0"] % 128 == 0
        assert it["rmin"] - it["a0"] in (0, 128) and it["cmin"] - it["b0"] in (0, 128)
    assert len(cover) == info.n_rtiles
    Ms = {0x100000 * (i + 1): M for i, (M, _, _) in enumerate(shapes)}
    for (A, a0, b0), ranges in cover.items():
        ranges.sort()
        pos = 0
        for r0, n in ranges:
            assert r0 == pos
            pos += n
        assert Ms[A] <= pos < Ms[A] + 128
    listed = set()
    for rt in rts:
        for p in range(int(rt["n_part"])):
            listed.add(int(rt["slab"]) + p * 256 * 1024)
    assert listed == slabs
    # per-workgroup lists: every item exactly once; the items of a shelf sit on one XCD's lanes and agree on its size
    lst = np.frombuffer(host[info.list_offset:info.list_offset + 4 * (info.n_ctas + 1 + info.n_items)].tobytes(), dtype="<i4")
    start, ids = lst[:info.n_ctas + 1], lst[info.n_ctas + 1:]
    assert start[0] == 0 and start[-1] == info.n_items and sorted(ids.tolist()) == list(range(info.n_items))
    load = np.array([sum(int(items["nk"][i]) for i in ids[start[c]:start[c + 1]]) for c in range(info.n_ctas)])
    assert load.max() <= 1.25 * load.mean(), (load.max(), load.mean())
    lanes = info.n_ctas // 8
    shelf_xcd, shelf_cnt = {}, {}
    for c in range(info.n_ctas):
        for i in ids[start[c]:start[c + 1]]:
            sh = int(items["sync_idx"][i])
            assert shelf_xcd.setdefault(sh, c // lanes) == c // lanes
            shelf_cnt[sh] = shelf_cnt.get(sh, 0) + 1
            assert 1 <= items["sync_n"][i] <= lanes
    for i in range(info.n_items):
        assert shelf_cnt[int(items["sync_idx"][i])] == items["sync_n"][i]
    assert not host[info.sync_offset:info.sync_offset + 4 * len(shelf_cnt)].any()          # the arrival counters start at zero


def test_host_side_dispatch_rules_without_a_gpu():
    """The planners that decide which kernel a shape runs on are host code (no launch): pinned here for the shapes of
    the step at 64 and 12 segments per GPU (a box without a GPU reports 256 CUs, the MI355X's count)."""
    L = lib.load()
    BF16 = 1
    # split K (mrmt3_gemm_nt_ws): only short inputs with K >= 2048 and >= 512 per split
    mpad = lambda m: -(-m // 128) * 128
    assert L.mrmt3_gemm_nt_workspace_bytes(3072, 512, 2048, BF16) == 4 * mpad(3072) * 512 * 4       # encoder d_wi, 12 segments
    assert L.mrmt3_gemm_nt_workspace_bytes(3072, 512, 6144, BF16) == 4 * mpad(3072) * 512 * 4       # cross k|v gradient
    assert L.mrmt3_gemm_nt_workspace_bytes(3000, 512, 2048, BF16) == 4 * mpad(3000) * 512 * 4       # ragged rows: padded slabs
    for shape in ((3072, 512, 1024), (3072, 512, 1152), (16384, 512, 2048), (65536, 512, 2048), (3072, 136, 2048),
                  (512, 512, 4096)):
        assert L.mrmt3_gemm_nt_workspace_bytes(*shape, BF16) == 0, shape
    assert L.mrmt3_gemm_nt_workspace_bytes(3072, 512, 2048, 0) == 0                                  # f32 operands: never
    # grouped weight gradients: widths on the 128 / 64 grid only (tests/test_fuzz_gpu.py found 576 admitted once)
    assert L.mrmt3_tn_group_ok(65536, 1152, 512, 1152, 512, 512) == 1
    assert L.mrmt3_tn_group_ok(65536, 576, 512, 576, 512, 512) == 0
    assert L.mrmt3_tn_group_ok(65536, 512, 520, 512, 520, 520) == 0
    assert L.mrmt3_tn_group_ok(512, 512, 512, 512, 512, 512) == 0                                    # too few token rows
    # scratch of the one-by-one weight gradient and of the norm backward are pure functions of the shape
    assert L.mrmt3_gemm_tn_workspace_bytes(65536, 2048, 512) == L.mrmt3_gemm_tn_splits(65536, 2048, 512) * 2048 * 512 * 4
    assert L.mrmt3_add_rmsnorm_bwd_workspace_bytes(65536, 512) > L.mrmt3_add_rmsnorm_bwd_partial_rows(65536) * 512 * 4
    assert L.mrmt3_add_rmsnorm_bwd_partial_rows(12288) >= 2048                                       # short inputs: >= ~2048 workgroups
