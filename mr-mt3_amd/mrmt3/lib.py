"""ctypes binding of libmrmt3_hip.so (include/mrmt3_hip.h).

The product path has NO CPU fallback: `load()` raises if the shared library is missing, and every
wrapper raises RuntimeError when the C ABI returns non-zero.  Tensors are passed as raw device
pointers; shapes/strides are explicit.  The stream is torch's current HIP stream.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import torch

F32, BF16 = 0, 1
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MRMT3_TOOL_LIB") or os.path.join(_HERE, "libmrmt3_hip.so")   # env: A/B a variant build (tuning only)
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "mrmt3_hip.h")
CSRC_DIR = os.path.join(os.path.dirname(_HERE), "csrc")
_lib = None

vp = C.c_void_p


def _header_text(path: str) -> str:
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def header_symbols(path: str = HEADER_PATH):
    """Names of every function the C header declares."""
    return sorted(set(re.findall(r"\b(mrmt3_[a-z0-9_]+)\s*\(", _header_text(path))))


_C_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "float": C.c_float, "size_t": C.c_size_t, "uint32_t": C.c_uint32,
              "uint64_t": C.c_uint64, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong}


def _ctype(decl: str, what: str):
    """ctypes type of one C type as the header spells it: scalars by value, `const char*` as c_char_p, every other
    pointer as an address, a pointer to a pointer (an out-parameter for a handle) as POINTER(c_void_p)."""
    stars = decl.count("*")
    words = decl.replace("*", " ").split()
    base = " ".join(w for w in words if w != "const")
    if stars == 0 and base == "void":
        return None
    if stars == 0 and base in _C_SCALARS:
        return _C_SCALARS[base]
    if stars == 1:
        return C.c_char_p if words == ["const", "char"] else C.c_void_p
    if stars == 2:
        return C.POINTER(C.c_void_p)
    raise TypeError(f"{what}: no ctypes mapping for the C type '{decl.strip()}'")


def header_signatures(path: str = HEADER_PATH) -> dict:
    """{name: (restype, argtypes)} of every prototype of the C header (plain C, one prototype per entry point)."""
    sigs = {}
    for ret, name, params in re.findall(r"([\w \t\*]+?)\b(mrmt3_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header_text(path)):
        args = []
        for prm in ([] if params.strip() == "void" else params.split(",")):
            m = re.fullmatch(r"\s*(.*?[\s\*])\w+\s*", prm, flags=re.S)       # type, then the parameter's name
            if m is None:
                raise TypeError(f"{name}: cannot parse the parameter '{prm.strip()}'")
            # (an f64 by value is a parameter type only — the matcher's tolerances; `_ctype` itself does not take it)
            args.append(C.c_double if m.group(1).split() == ["double"] else _ctype(m.group(1), name))
        sigs[name] = (_ctype(ret, name), args)
    if set(sigs) != set(header_symbols(path)):
        raise TypeError("unparsed prototypes: %s" % sorted(set(sigs) ^ set(header_symbols(path))))
    return sigs


_SIGS = header_signatures()          # applied by load(): the header is the one place a signature is written down


def build(verbose: bool = False, diag: bool = True) -> str:
    """Compile csrc/*.hip for gfx950 into libmrmt3_hip.so (hipcc cross-compiles without a GPU) and, with `diag`, the
    -DMRMT3_DIAG twin libmrmt3_hip_diag.so that profiles/tools load (never the product path)."""
    for target in (["all"], ["diag"]) if diag else (["all"],):
        r = subprocess.run(["make", "-C", CSRC_DIR, "-j8"] + target, capture_output=True, text=True)
        if verbose or r.returncode != 0:
            print(r.stdout[-4000:], r.stderr[-4000:])
        if r.returncode != 0:
            raise RuntimeError("building libmrmt3_hip.so failed (make %s)" % target[0])
    return LIB_PATH


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the MI355X kernels are the only implementation of this path "
            "(no CPU fallback). Run `python __graft_entry__.py` / `make -C mr-mt3_amd/csrc` first.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        if os.environ.get("MRMT3_TOOL_LIB") and not hasattr(lib, name):
            continue                       # tuning only: an older variant build under A/B may lack newer entry points
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if not os.environ.get("MRMT3_TOOL_LIB") and lib.mrmt3_version() < MIN_VERSION:
        raise RuntimeError(f"{LIB_PATH} is version {lib.mrmt3_version()}, this binding needs >= {MIN_VERSION}: "
                           "a stale build — run `make -C mr-mt3_amd/csrc`")
    _lib = lib
    return lib


MIN_VERSION = 129
COUNTER_NAMES = ("gemm_nt_tile", "gemm_nt8", "gemm_nt_geglu", "tn_group", "tn8", "tn_tile", "attn_fwd", "attn_bwd",
                 "attn_bwd_onepass", "attn_f32", "tn_f32", "gemm_nt_splitk", "gemm_nt_addnorm", "gemm_nt_normbwd",
                 "gemm_nt_geglubwd", "attn_fwd_varlen", "attn_bwd_varlen", "logmel_wave", "logmel_general")


def set_knob(name: str, value: int):
    """Override a dispatch / tuning switch of the C library in-process (mrmt3_set_knob): `name` is the environment
    variable's name (MRMT3_ROWS_BM, MRMT3_GEMM8, ...), `value` the integer it would hold.  The library reads its knobs from
    the environment once per process; tests and tuning tools switch them through this call."""
    _check(load().mrmt3_set_knob(name.encode(), int(value)), "set_knob")


def reset_knobs():
    """Drop every override; each knob is re-read from the environment at its next use."""
    _check(load().mrmt3_reset_knobs(), "reset_knobs")


def dispatch_counts(reset: bool = False) -> dict:
    """Launches per kernel family since the process started / the last reset (mrmt3_dispatch_counts; diagnostics)."""
    arr = (C.c_ulonglong * len(COUNTER_NAMES))()
    n = load().mrmt3_dispatch_counts(arr, len(COUNTER_NAMES), int(reset))
    assert n == len(COUNTER_NAMES), "lib.COUNTER_NAMES is out of step with MRMT3_CNT_N"
    return {k: int(arr[i]) for i, k in enumerate(COUNTER_NAMES)}


# Optional per-launch timing used by bench.py's roofline leg: when PROFILE is a list, the wrappers of
# the heavy kernels bracket their launch with events on the current stream and append
# (family, algorithmic_work, unit, start_event, end_event).
PROFILE = None
PROFILE_BYTES = {}      # family -> algorithmic bytes (operands read once + output written once) while PROFILE is on


class _Timed:
    def __init__(self, family, work, unit, executed=None):
        self.args = (family, work, unit)
        self.executed = executed     # optional second price of the same launch (family "<name>@executed")

    def __enter__(self):
        if PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if PROFILE is not None:
            self.e1.record()
            PROFILE.append(self.args + (self.e0, self.e1))
            if self.executed is not None:
                PROFILE.append((self.args[0] + "@executed", self.executed, self.args[2], self.e0, self.e1))
        return False


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed (code {rc}): {load().mrmt3_last_error().decode()}")


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("mrmt3 kernels need device tensors (no CPU fallback)")


# ---- thin wrappers (shape checks live in the C library) -----------------------------------------

def logmel(audio, tables, valid_frames=None, normalize=True, out_bf16=False):
    _dev(audio)
    B, n = audio.shape
    hop, n_mels = tables["hop"], tables["n_mels"]
    frames = -(-n // hop)
    out = torch.empty(B, frames, n_mels, device=audio.device, dtype=torch.bfloat16 if out_bf16 else torch.float32)
    with _Timed("logmel", audio.numel() * 4 + out.numel() * out.element_size(), "B"):
        _check(load().mrmt3_logmel_fwd(_p(audio), B, n, hop, _p(tables["window"]), _p(tables["twiddle"]),
                                       _p(tables["fb_start"]), _p(tables["fb_cnt"]), _p(tables["fb_w"]), n_mels,
                                       tables["max_taps"], _p(valid_frames), int(normalize), int(out_bf16), _p(out),
                                       _stream()), "logmel_fwd")
    return out


def logmel_crops(audio, seg_start, n_samples, tables, valid_frames=None, normalize=True, out_bf16=False):
    """audio [total] f32 (one recording), seg_start [B] int64 sample offsets -> [B, ceil(n/hop), n_mels]."""
    _dev(audio, seg_start)
    assert audio.dim() == 1 and audio.dtype == torch.float32 and audio.is_contiguous()
    assert seg_start.dtype == torch.int64 and seg_start.is_contiguous()
    assert valid_frames is None or (valid_frames.dtype == torch.int32 and valid_frames.numel() == seg_start.numel())
    B = seg_start.numel()
    hop, n_mels = tables["hop"], tables["n_mels"]
    frames = -(-n_samples // hop)
    out = torch.empty(B, frames, n_mels, device=audio.device, dtype=torch.bfloat16 if out_bf16 else torch.float32)
    with _Timed("logmel", B * n_samples * 4 + out.numel() * out.element_size(), "B"):
        _check(load().mrmt3_logmel_crops_fwd(_p(audio), audio.numel(), _p(seg_start), B, n_samples, hop,
                                             _p(tables["window"]), _p(tables["twiddle"]), _p(tables["fb_start"]),
                                             _p(tables["fb_cnt"]), _p(tables["fb_w"]), n_mels, tables["max_taps"],
                                             _p(valid_frames), int(normalize), int(out_bf16), _p(out), _stream()),
               "logmel_crops_fwd")
    return out


def logmel_mix(pool, src_start, src_end, src_gain, n_samples, tables, valid_frames=None, normalize=True, out_bf16=False):
    """pool [total] f32 (stems end to end); src_start / src_end [B, n_src] int64 pool offsets (first sample of the crop,
    one past the stem's last sample), src_gain [B, n_src] f32 (0: the source is not read) -> [B, ceil(n/hop), n_mels]:
    the log-mel of the rows' gain-weighted stem sums (include/mrmt3_hip.h: mrmt3_logmel_mix_fwd)."""
    _dev(pool, src_start, src_end, src_gain, valid_frames)
    assert pool.dim() == 1 and pool.dtype == torch.float32 and pool.is_contiguous()
    assert src_start.dim() == 2 and src_start.dtype == torch.int64 and src_start.is_contiguous()
    assert src_end.shape == src_start.shape and src_end.dtype == torch.int64 and src_end.is_contiguous()
    assert src_gain.shape == src_start.shape and src_gain.dtype == torch.float32 and src_gain.is_contiguous()
    B, n_src = src_start.shape
    assert valid_frames is None or (valid_frames.dtype == torch.int32 and valid_frames.is_contiguous()
                                    and valid_frames.numel() == B)
    hop, n_mels = tables["hop"], tables["n_mels"]
    frames = -(-n_samples // hop)
    out = torch.empty(B, frames, n_mels, device=pool.device, dtype=torch.bfloat16 if out_bf16 else torch.float32)
    with _Timed("logmel", B * n_samples * 4 * n_src + out.numel() * out.element_size(), "B"):
        _check(load().mrmt3_logmel_mix_fwd(_p(pool), pool.numel(), _p(src_start), _p(src_end), _p(src_gain), n_src, B,
                                           n_samples, hop, _p(tables["window"]), _p(tables["twiddle"]),
                                           _p(tables["fb_start"]), _p(tables["fb_cnt"]), _p(tables["fb_w"]), n_mels,
                                           tables["max_taps"], _p(valid_frames), int(normalize), int(out_bf16), _p(out),
                                           _stream()), "logmel_mix_fwd")
    return out


def resample_mix(pool, src_pos, src_begin, src_end, src_step, src_gain, src_filt, n_samples, filt, valid_samples=None):
    """pool [total] f32 (stems end to end); src_pos / src_begin / src_end / src_step [B, n_src] int64 (32.32 position of
    output 0, the stem's first sample, one past its last, 32.32 input samples per output sample), src_gain [B, n_src] f32
    (0: not read), src_filt [B, n_src] int32 (table index, -1: pass-through); filt [n_filt, 513, n_taps] f32 polyphase
    tables; valid_samples [B] int64 or None -> [B, n_samples] f32 rows, resampled and mixed
    (include/mrmt3_hip.h: mrmt3_resample_mix_fwd)."""
    _dev(pool, src_pos, src_begin, src_end, src_step, src_gain, src_filt, filt, valid_samples)
    assert pool.dim() == 1 and pool.dtype == torch.float32 and pool.is_contiguous()
    assert src_pos.dim() == 2 and src_pos.dtype == torch.int64 and src_pos.is_contiguous()
    for t in (src_begin, src_end, src_step):
        assert t.shape == src_pos.shape and t.dtype == torch.int64 and t.is_contiguous()
    assert src_gain.shape == src_pos.shape and src_gain.dtype == torch.float32 and src_gain.is_contiguous()
    assert src_filt.shape == src_pos.shape and src_filt.dtype == torch.int32 and src_filt.is_contiguous()
    assert filt.dim() == 3 and filt.shape[1] == 513 and filt.dtype == torch.float32 and filt.is_contiguous()
    B, n_src = src_pos.shape
    assert valid_samples is None or (valid_samples.dtype == torch.int64 and valid_samples.is_contiguous()
                                     and valid_samples.numel() == B)
    out = torch.empty(B, int(n_samples), device=pool.device, dtype=torch.float32)
    _check(load().mrmt3_resample_mix_fwd(_p(pool), pool.numel(), _p(src_pos), _p(src_begin), _p(src_end), _p(src_step),
                                         _p(src_gain), _p(src_filt), n_src, B, int(n_samples), _p(filt), filt.shape[0],
                                         filt.shape[2], _p(valid_samples), _p(out), _stream()), "resample_mix_fwd")
    return out


def resample_launches(reset: bool = False) -> int:
    """Launches of `resample_mix` since the process started / the last reset (mrmt3_resample_launches): the resampler's
    dispatch counter, kept apart from `dispatch_counts` so that an untouched step counts exactly as before."""
    return int(load().mrmt3_resample_launches(int(reset)))


LABEL_CAPACITY = 2048        # events of one row's window, and tie pairs, that mrmt3_label_rows_fwd holds (an ABI constant)


def label_rows(note_times, note_meta, n_stems, keep, start_frame, n_frames, total_frames, scale, shift, codec,
               event_length=1024):
    """note_times [N, 2] f64 and note_meta [N, 4] int32 (a `mrmt3.labels.NoteTable` on the device); keep [B] int64 holding
    the uint64 stem masks, start_frame / n_frames / total_frames [B] int64, scale [B] f64, shift [B] int32; `codec` a
    `mrmt3.labels.LabelCodec` -> (targets [B, event_length] int64 in `pad_targets` form, status [B] int32, 0 where the row
    is exact) (include/mrmt3_hip.h: mrmt3_label_rows_fwd)."""
    _dev(note_times, note_meta, keep, start_frame, n_frames, total_frames, scale, shift)
    N = note_meta.shape[0]
    assert note_times.shape == (N, 2) and note_times.dtype == torch.float64 and note_times.is_contiguous()
    assert note_meta.shape == (N, 4) and note_meta.dtype == torch.int32 and note_meta.is_contiguous()
    B = keep.numel()
    for t in (keep, start_frame, n_frames, total_frames):
        assert t.shape == (B,) and t.dtype == torch.int64 and t.is_contiguous()
    assert scale.shape == (B,) and scale.dtype == torch.float64 and scale.is_contiguous()
    assert shift.shape == (B,) and shift.dtype == torch.int32 and shift.is_contiguous()
    targets = torch.empty(B, int(event_length), device=keep.device, dtype=torch.int64)
    status = torch.empty(B, device=keep.device, dtype=torch.int32)
    _check(load().mrmt3_label_rows_fwd(
        _p(note_times) if N else None, _p(note_meta) if N else None, N, int(n_stems), _p(keep), _p(start_frame),
        _p(n_frames), _p(total_frames), _p(scale), _p(shift), B, codec.pitch_base, codec.velocity_base, codec.tie_token,
        codec.program_base, codec.drum_base, codec.max_shift_steps,
        codec.steps_per_second, codec.sample_rate, codec.hop, int(event_length), codec.num_special_tokens, _p(targets),
        _p(status), _stream()), "label_rows_fwd")
    return targets, status


LABEL_MAX_PARTS = 4          # parts of one row of mrmt3_label_rows_parts_fwd (LB_MAX_PARTS, an ABI constant)


def label_rows_parts(note_times, note_meta, note_first, note_count, keep, delay_frames, scale, shift, start_frame, n_frames,
                     total_frames, codec, event_length=1024):
    """Rows of virtual tracks.  note_times [N, 2] f64 and note_meta [N, 4] int32: the note arena on the device;
    note_first / note_count [B, P] int32, keep (uint64 masks) / delay_frames [B, P] int64, scale [B, P] f64, shift [B, P]
    int32, 1 <= P <= LABEL_MAX_PARTS; start_frame / n_frames / total_frames [B] int64 -> (targets [B, event_length] int64,
    status [B] int32) as `label_rows` (include/mrmt3_hip.h: mrmt3_label_rows_parts_fwd)."""
    _dev(note_times, note_meta, note_first, note_count, keep, delay_frames, scale, shift, start_frame, n_frames, total_frames)
    N = note_meta.shape[0]
    assert note_times.shape == (N, 2) and note_times.dtype == torch.float64 and note_times.is_contiguous()
    assert note_meta.shape == (N, 4) and note_meta.dtype == torch.int32 and note_meta.is_contiguous()
    assert keep.dim() == 2
    B, P = keep.shape
    for t, dt in ((note_first, torch.int32), (note_count, torch.int32), (keep, torch.int64), (delay_frames, torch.int64),
                  (scale, torch.float64), (shift, torch.int32)):
        assert t.shape == (B, P) and t.dtype == dt and t.is_contiguous()
    for t in (start_frame, n_frames, total_frames):
        assert t.shape == (B,) and t.dtype == torch.int64 and t.is_contiguous()
    targets = torch.empty(B, int(event_length), device=keep.device, dtype=torch.int64)
    status = torch.empty(B, device=keep.device, dtype=torch.int32)
    _check(load().mrmt3_label_rows_parts_fwd(
        _p(note_times) if N else None, _p(note_meta) if N else None, N, P, _p(note_first), _p(note_count), _p(keep),
        _p(delay_frames), _p(scale), _p(shift), _p(start_frame), _p(n_frames), _p(total_frames), B, codec.pitch_base,
        codec.velocity_base, codec.tie_token, codec.program_base, codec.drum_base, codec.max_shift_steps,
        codec.steps_per_second, codec.sample_rate, codec.hop, int(event_length), codec.num_special_tokens, _p(targets),
        _p(status), _stream()), "label_rows_parts_fwd")
    return targets, status


def label_launches(reset: bool = False) -> int:
    """Launches of `label_rows` and `label_rows_parts` since the process started / the last reset (mrmt3_label_launches)."""
    return int(load().mrmt3_label_launches(int(reset)))


NOTES_CAPACITY = 4096        # notes of one recording that may sound at once in mrmt3_notes_decode_fwd (MRMT3_NOTES_CAPACITY)


def notes_decode(grammar, ids, seg_first, start_time, limit, velocity_of_bin, steps_per_second, logp=None):
    """ids [rows, ld] int64 as the decoder returns them (column 0 the start token), logp [rows, ld] f32 beside it or None;
    seg_first [n_rec + 1] int32, start_time / limit [rows] f64, velocity_of_bin [n_velocity] int32, all on the device;
    `grammar` a `mrmt3.grammar.EventGrammar` (the id ranges), `steps_per_second` the codec's -> dict of device tensors:
    n_notes, invalid, dropped, status [n_rec] int32, total_time [n_rec] f64, times [rows * (ld - 1), 2] f64,
    meta [rows * (ld - 1), 4] int32 and, with `logp`, logc [rows * (ld - 1)] f32; recording r's notes start at entry
    seg_first[r] * (ld - 1) (include/mrmt3_hip.h: mrmt3_notes_decode_fwd)."""
    _dev(ids, seg_first, start_time, limit, velocity_of_bin, logp)
    assert ids.dim() == 2 and ids.dtype == torch.int64 and ids.is_contiguous()
    rows, ld = ids.shape
    assert logp is None or (logp.shape == ids.shape and logp.dtype == torch.float32 and logp.is_contiguous())
    assert seg_first.dim() == 1 and seg_first.dtype == torch.int32 and seg_first.is_contiguous()
    n_rec = seg_first.numel() - 1
    for t in (start_time, limit):
        assert t.shape == (rows,) and t.dtype == torch.float64 and t.is_contiguous()
    assert velocity_of_bin.shape == (grammar.n_velocity,) and velocity_of_bin.dtype == torch.int32
    assert velocity_of_bin.is_contiguous()
    if steps_per_second != int(steps_per_second):
        raise ValueError(f"notes_decode needs a whole steps_per_second, got {steps_per_second!r}")
    g = grammar.c_struct()
    g.steps_per_second = int(steps_per_second)
    dev, cap = ids.device, max(rows * (ld - 1), 0)
    out = {k: torch.empty(max(n_rec, 0), device=dev, dtype=torch.int32) for k in ("n_notes", "invalid", "dropped", "status")}
    out["total_time"] = torch.empty(max(n_rec, 0), device=dev, dtype=torch.float64)
    out["times"] = torch.empty(cap, 2, device=dev, dtype=torch.float64)
    out["meta"] = torch.empty(cap, 4, device=dev, dtype=torch.int32)
    out["logc"] = None if logp is None else torch.empty(cap, device=dev, dtype=torch.float32)
    _check(load().mrmt3_notes_decode_fwd(C.byref(g), _p(ids), _p(logp), rows, ld, _p(seg_first), n_rec, _p(start_time),
                                         _p(limit), _p(velocity_of_bin), _p(out["n_notes"]), _p(out["invalid"]),
                                         _p(out["dropped"]), _p(out["status"]), _p(out["total_time"]), _p(out["times"]),
                                         _p(out["meta"]), _p(out["logc"]), _stream()), "notes_decode_fwd")
    return out


def notes_launches(reset: bool = False) -> int:
    """Launches of `notes_decode` since the process started / the last reset (mrmt3_notes_launches)."""
    return int(load().mrmt3_notes_launches(int(reset)))


def _note_lists(who, ref_times, ref_meta, est_times, est_meta, ref_idx, ref_first, est_idx, est_first) -> int:
    """The check `note_match` and `note_frames` share, before anything touches the device: two note tables, two lists, two
    `first` arrays.  A ValueError that names the wrapper `who`; returns n_prob."""
    for name, times, meta in (("ref", ref_times, ref_meta), ("est", est_times, est_meta)):
        n = meta.shape[0]
        if tuple(times.shape) != (n, 2) or times.dtype != torch.float64 or not times.is_contiguous():
            raise ValueError(f"{who}: {name}_times must be contiguous [n, 2] f64, got {tuple(times.shape)} {times.dtype}")
        if meta.dim() != 2 or meta.shape[1] != 4 or meta.dtype != torch.int32 or not meta.is_contiguous():
            raise ValueError(f"{who}: {name}_meta must be contiguous [n, 4] int32, got {tuple(meta.shape)} {meta.dtype}")
        if n >= 1 << 31:
            raise ValueError(f"{who}: {n} {name} notes, the note counts must be in [0, 2^31)")
    for name, t in (("ref_idx", ref_idx), ("est_idx", est_idx), ("ref_first", ref_first), ("est_first", est_first)):
        if t.dim() != 1 or t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be contiguous 1-D int32, got {tuple(t.shape)} {t.dtype}")
    n_prob = ref_first.numel() - 1
    if n_prob <= 0 or est_first.numel() != n_prob + 1:
        raise ValueError(f"{who}: ref_first and est_first must both be [n_prob + 1] with n_prob > 0, got "
                         f"{ref_first.numel()} and {est_first.numel()} entries")
    return n_prob


def _or_spare(dev):
    """t -> its pointer, or that of a spare block where t is empty (an empty tensor's pointer is null, which the C library
    refuses)."""
    spare = torch.empty(4, 4, device=dev, dtype=torch.int32)
    return lambda t: _p(t) if t.numel() else _p(spare)


def note_match(ref_times, ref_meta, est_times, est_meta, ref_idx, ref_first, est_idx, est_first, prob_flags, pitch_lo,
               pitch_hi, onset_tol=0.05, offset_ratio=0.2, offset_min_tol=0.05):
    """ref_times / est_times [n, 2] f64 and ref_meta / est_meta [n, 4] int32 (note tables: a `mrmt3.labels.NoteTable` on the
    device, the output of `notes_decode`); ref_idx [Lr] / est_idx [Le] int32, the entries of every problem's two lists, each
    in onset order; ref_first / est_first [n_prob + 1] int32; prob_flags [n_prob] int32 (bit 0: offsets on, bits 8..: the
    pitch table); pitch_lo / pitch_hi [n_tables, 128] int32, all on the device -> (matched [n_prob] int32, match [Le] int32,
    status [n_prob] int32).  ONE launch for every problem; Lr and Le are taken from the list tensors' lengths, no read-back
    (include/mrmt3_hip.h: mrmt3_note_match_fwd).  A malformed argument is a ValueError, before anything is launched."""
    n_prob = _note_lists("note_match", ref_times, ref_meta, est_times, est_meta, ref_idx, ref_first, est_idx, est_first)
    if prob_flags.dim() != 1 or prob_flags.dtype != torch.int32 or not prob_flags.is_contiguous() or prob_flags.numel() != n_prob:
        raise ValueError(f"note_match: prob_flags must be contiguous [n_prob = {n_prob}] int32, got "
                         f"{tuple(prob_flags.shape)} {prob_flags.dtype}")
    for name, t in (("pitch_lo", pitch_lo), ("pitch_hi", pitch_hi)):
        if t.dim() != 2 or t.shape[1] != 128 or t.shape != pitch_lo.shape or t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError(f"note_match: {name} must be contiguous [n_tables, 128] int32, got {tuple(t.shape)} {t.dtype}")
    _dev(ref_times, ref_meta, est_times, est_meta, ref_idx, ref_first, est_idx, est_first, prob_flags, pitch_lo, pitch_hi)
    dev, Lr, Le = prob_flags.device, ref_idx.numel(), est_idx.numel()
    matched = torch.empty(n_prob, device=dev, dtype=torch.int32)
    status = torch.empty(n_prob, device=dev, dtype=torch.int32)
    match = torch.empty(Le, device=dev, dtype=torch.int32)
    lib = load()
    words = int(lib.mrmt3_note_match_workspace_bytes(Lr, Le)) // 4
    if words == 0 and (Lr or Le):
        raise ValueError(f"note_match: list lengths {Lr}, {Le} are beyond the kernel's 2^30 entries")
    ws = torch.empty(max(words, 1), device=dev, dtype=torch.int32)
    ptr = _or_spare(dev)
    _check(lib.mrmt3_note_match_fwd(ptr(ref_times), ptr(ref_meta), ref_meta.shape[0], ptr(est_times), ptr(est_meta),
                                    est_meta.shape[0], ptr(ref_idx), _p(ref_first), ptr(est_idx), _p(est_first),
                                    ptr(prob_flags), n_prob, _p(pitch_lo), _p(pitch_hi), pitch_lo.shape[0], float(onset_tol),
                                    float(offset_ratio), float(offset_min_tol), _p(matched), ptr(match), _p(status), _p(ws),
                                    _stream()), "note_match_fwd")
    return matched, match, status


def note_match_launches(reset: bool = False) -> int:
    """Launches of `note_match` since the process started / the last reset (mrmt3_note_match_launches)."""
    return int(load().mrmt3_note_match_launches(int(reset)))


FRAMES_MAX = (1 << 31) - 64      # the largest n_frames of mrmt3_note_frames_fwd


def note_frames(ref_times, ref_meta, est_times, est_meta, ref_idx, ref_first, est_idx, est_first, fps, n_frames,
                with_roll=False):
    """Tables, lists and `first` arrays as `note_match` takes them (the lists in any order), fps frames a second, n_frames
    the length of the rolls -> (counts [n_prob, 3] int64: tp, n_ref, n_est; skipped [n_prob, 2] int32; clipped [n_prob, 2]
    int32) and, with `with_roll`, roll [n_prob, 2, 128, W] int32 (W = ceil(n_frames / 32) words of 32 frames, frame f is bit
    f % 32 of word f // 32).  ONE launch for every problem, no read-back (include/mrmt3_hip.h: mrmt3_note_frames_fwd).
    An argument the C library would refuse is a ValueError here, before anything is launched."""
    import math
    if isinstance(fps, bool) or not isinstance(fps, (int, float)) or not math.isfinite(fps) or fps <= 0:
        raise ValueError(f"note_frames: fps must be finite and > 0, got {fps!r}")
    if isinstance(n_frames, bool) or int(n_frames) != n_frames or not 1 <= int(n_frames) <= FRAMES_MAX:
        raise ValueError(f"note_frames: n_frames must be a whole number in [1, 2^31 - 64], got {n_frames!r}")
    n_prob = _note_lists("note_frames", ref_times, ref_meta, est_times, est_meta, ref_idx, ref_first, est_idx, est_first)
    _dev(ref_times, ref_meta, est_times, est_meta, ref_idx, ref_first, est_idx, est_first)
    dev, n_frames = ref_first.device, int(n_frames)
    counts = torch.empty(n_prob, 3, device=dev, dtype=torch.int64)
    skipped = torch.empty(n_prob, 2, device=dev, dtype=torch.int32)
    clipped = torch.empty(n_prob, 2, device=dev, dtype=torch.int32)
    roll = torch.empty(n_prob, 2, 128, -(-n_frames // 32), device=dev, dtype=torch.int32) if with_roll else None
    ptr = _or_spare(dev)
    _check(load().mrmt3_note_frames_fwd(ptr(ref_times), ptr(ref_meta), ref_meta.shape[0], ptr(est_times), ptr(est_meta),
                                        est_meta.shape[0], ptr(ref_idx), _p(ref_first), ptr(est_idx), _p(est_first), n_prob,
                                        float(fps), n_frames, _p(counts), _p(skipped), _p(clipped), _p(roll), None, _stream()),
           "note_frames_fwd")
    return (counts, skipped, clipped, roll) if with_roll else (counts, skipped, clipped)


def note_frames_launches(reset: bool = False) -> int:
    """Launches of `note_frames` since the process started / the last reset (mrmt3_note_frames_launches)."""
    return int(load().mrmt3_note_frames_launches(int(reset)))


def gemm_nt(a, b, out=None, out_dtype=None, accumulate=False):
    """out[M,N] (+)= a[M,K] @ b[N,K]^T ; a/b are 2-D, last dim contiguous (row stride may exceed K)."""
    _dev(a, b)
    M, K = a.shape
    N = b.shape[0]
    assert b.shape[1] == K and a.stride(1) == 1 and b.stride(1) == 1
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=out_dtype or a.dtype)
    assert out.stride(1) == 1
    fam = "gemm_nt_bf16" if a.dtype == torch.bfloat16 else "gemm_nt_f32"
    if PROFILE is not None:
        PROFILE_BYTES[fam] = PROFILE_BYTES.get(fam, 0.0) + (M * K + N * K) * a.element_size() + M * N * out.element_size()
    # short inputs with a long K (the encoder at 12 segments per GPU) run split over K through a scratch buffer
    key = (M, N, K, a.dtype)
    ws_bytes = _NT_WS.get(key)
    if ws_bytes is None:
        ws_bytes = _NT_WS[key] = int(load().mrmt3_gemm_nt_workspace_bytes(M, N, K, _dt(a)))
    with _Timed(fam, 2.0 * M * N * K, "FLOP"):
        if ws_bytes:
            ws = workspace(ws_bytes, a.device)
            _check(load().mrmt3_gemm_nt_ws(_p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), M, N, K, _dt(a),
                                           _dt(out), int(accumulate), _p(ws), ws.numel(), _stream()), "gemm_nt_ws")
        else:
            _check(load().mrmt3_gemm_nt(_p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), M, N, K, _dt(a),
                                        _dt(out), int(accumulate), _stream()), "gemm_nt")
    return out


_NT_WS = {}          # (M, N, K, dtype) -> scratch bytes of the split-K form (0: the shape does not split)


_ws_cache = {}


_ws_retired = []


def workspace(nbytes: int, device) -> torch.Tensor:
    # one scratch buffer per (device, stream): kernels on different streams may run concurrently
    key = (device.index if hasattr(device, "index") else 0, torch.cuda.current_stream().cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            # kernels already queued on that stream may still be using the old buffer, and the caching allocator
            # would hand its memory to the CURRENT stream: keep it (growth stops after the first steps)
            _ws_retired.append(buf)
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


class _TnGSite(C.Structure):          # = mrmt3_tn_gsite
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("C", C.c_void_p)] + \
               [(n, C.c_int32) for n in ("lda", "ldb", "ldc", "M", "N1", "N2", "accumulate", "pad")]


class _TnGInfo(C.Structure):          # = mrmt3_tn_group_info
    _fields_ = [(n, C.c_int32) for n in ("n_ctas", "n_items", "n_rtiles", "rounds")] + \
               [(n, C.c_uint64) for n in ("rtile_offset", "list_offset", "sync_offset", "table_bytes", "slab_bytes")]


class _PinnedTable:
    """Page-locked host bytes from the library's own allocator (torch's pinned-memory cache polls events when it
    allocates, which is illegal while a stream of the thread is capturing)."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.ptr = load().mrmt3_host_alloc(self.nbytes)
        if not self.ptr:
            raise RuntimeError("mrmt3_host_alloc failed: " + load().mrmt3_last_error().decode())

    def __del__(self):
        try:
            if self.ptr:
                load().mrmt3_host_free(C.c_void_p(self.ptr))
        except Exception:
            pass
        self.ptr = None


class TnGroup:
    """The weight-gradient GEMMs of a whole gradient bucket (or of the whole backward) in ONE MFMA launch + ONE reduce
    (mrmt3_tn_group_plan / mrmt3_tn_group_run).  `add()` only records the operands (and keeps them alive); `flush()`
    plans the items on the host — cached per set of (addresses, shapes) — and launches on the current stream; the table
    reaches the device through an async copy from page-locked memory (a memcpy node when the step is being captured:
    the replays re-send the same bytes).  Gradients are complete after flush().

    Nothing is allocated from the host while a stream is capturing: every eager plan leaves a spare page-locked table
    of its size behind, which the capture of the same step (same shapes, new addresses) picks up."""

    def __init__(self):
        self._sites = []
        self._plans = {}          # key -> dict(host, table, info, flops, slab, captured)
        self._spare = []          # page-locked tables ready for a plan made under capture
        self._slab = None
        self.last_info = None

    @staticmethod
    def ok(a, b, out):
        return (a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and out.dtype == torch.float32 and
                a.stride(1) == 1 and b.stride(1) == 1 and out.stride(1) == 1 and
                bool(load().mrmt3_tn_group_ok(a.shape[0], a.shape[1], b.shape[1], a.stride(0), b.stride(0), out.stride(0))))

    def add(self, a, b, out, accumulate=True):
        assert a.shape[0] == b.shape[0] and tuple(out.shape) == (a.shape[1], b.shape[1])
        if any(o.data_ptr() == out.data_ptr() for _, _, o, _ in self._sites):
            # the same gradient twice in one launch (a weight used twice per backward): its tiles would be reduced into
            # C by different workgroups without an order.  Finish the first use before the second is queued.
            self.flush()
        self._sites.append((a, b, out, int(bool(accumulate))))

    def __len__(self):
        return len(self._sites)

    def clear(self):
        """Forget what was recorded without launching it (the operands of work that never ran); plans and spares stay."""
        self._sites.clear()

    def _host_table(self, nbytes, capturing):
        if not capturing:
            return _PinnedTable(nbytes)         # (the spares are for captures only: an eager plan must not use one up)
        fit = [i for i, h in enumerate(self._spare) if h.nbytes >= nbytes]
        if not fit:
            raise RuntimeError("TnGroup: no page-locked table of %d bytes was prepared before the capture "
                               "(run the step eagerly once with the same shapes first)" % nbytes)
        return self._spare.pop(min(fit, key=lambda i: self._spare[i].nbytes))

    def flush(self):
        if not self._sites:
            return
        try:
            self._flush()
        finally:
            self._sites.clear()        # also when planning / launching raised: the sites must not leak into the next flush

    def _flush(self):
        L = load()
        dev = self._sites[0][0].device
        key = tuple((a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), o.data_ptr(), o.stride(0), a.shape[0],
                     a.shape[1], b.shape[1], acc) for a, b, o, acc in self._sites)
        ent = self._plans.get(key)
        if ent is not None and ent["slab"] is not self._slab:
            ent = None
        if ent is None:
            capturing = torch.cuda.is_current_stream_capturing()
            n = len(self._sites)
            arr = (_TnGSite * n)()
            flops = 0.0
            for i, (a, b, o, acc) in enumerate(self._sites):
                arr[i] = _TnGSite(a.data_ptr(), b.data_ptr(), o.data_ptr(), a.stride(0), b.stride(0), o.stride(0),
                                  a.shape[0], a.shape[1], b.shape[1], acc, 0)
                flops += 2.0 * a.shape[0] * a.shape[1] * b.shape[1]
            info = _TnGInfo()
            _check(L.mrmt3_tn_group_plan(arr, n, None, None, 0, C.byref(info)), "tn_group_plan (sizing)")
            if self._slab is None or self._slab.numel() < info.slab_bytes:
                self._slab = None
                self._slab = torch.empty(int(info.slab_bytes), device=dev, dtype=torch.uint8)
            if os.environ.get("MRMT3_TN_GROUP_DEBUG"):
                print("TnGroup plan: sites", n, "table", int(info.table_bytes), "capturing", capturing, "spares",
                      [h.nbytes for h in self._spare], "plans", len(self._plans), flush=True)
            host = self._host_table(int(info.table_bytes), capturing)
            _check(L.mrmt3_tn_group_plan(arr, n, _p(self._slab), C.c_void_p(host.ptr), host.nbytes, C.byref(info)),
                   "tn_group_plan")
            table = torch.empty(int(info.table_bytes), device=dev, dtype=torch.uint8)
            ent = dict(host=host, table=table, info=info, flops=flops, slab=self._slab, captured=capturing)
            if not capturing:
                # one spare per eager plan: a step with several joins (one per gradient bucket) needs as many tables
                # when it is captured
                self._spare.append(_PinnedTable(int(info.table_bytes)))
                if len(self._spare) > 64:
                    self._spare.pop(0)
                eager = [k for k, e in self._plans.items() if not e["captured"]]
                if len(eager) >= 128:                          # eager address churn (steady state reuses addresses)
                    torch.cuda.current_stream().synchronize()  # their table copies have been consumed
                    for k in eager:
                        del self._plans[k]
            self._plans[key] = ent
        with _Timed("gemm_tn_bf16", ent["flops"], "FLOP"):
            _check(L.mrmt3_tn_group_run(_p(ent["table"]), C.c_void_p(ent["host"].ptr), C.byref(ent["info"]), _stream()),
                   "tn_group_run")
        self.last_info = ent["info"]


def gemm_tn_f32(a, b, out, accumulate=False):
    """out[N1,N2] (+)= a[M,N1]^T @ b[M,N2], everything f32 (the fp32 training / parity path)."""
    _dev(a, b, out)
    M, N1 = a.shape
    N2 = b.shape[1]
    assert b.shape[0] == M and tuple(out.shape) == (N1, N2)
    assert a.dtype == b.dtype == out.dtype == torch.float32 and a.stride(1) == 1 and b.stride(1) == 1 and out.stride(1) == 1
    with _Timed("gemm_tn_f32", 2.0 * M * N1 * N2, "FLOP"):
        _check(load().mrmt3_gemm_tn_f32(_p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), M, N1, N2,
                                        int(accumulate), _stream()), "gemm_tn_f32")
    return out


def gemm_tn(a, b, out, accumulate=False):
    """out[N1,N2] (+)= a[M,N1]^T @ b[M,N2]  (bf16 in, f32 out), on the current stream."""
    _dev(a, b, out)
    M, N1 = a.shape
    N2 = b.shape[1]
    assert b.shape[0] == M and a.stride(1) == 1 and b.stride(1) == 1 and out.stride(1) == 1
    lib = load()
    ws = workspace(lib.mrmt3_gemm_tn_workspace_bytes(M, N1, N2), a.device)
    with _Timed("gemm_tn_bf16", 2.0 * M * N1 * N2, "FLOP"):
        _check(lib.mrmt3_gemm_tn(_p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), M, N1, N2,
                                 int(accumulate), _p(ws), ws.numel(), _stream()), "gemm_tn")
    return out


def add_rmsnorm_fwd(x0, y, w, eps, xn_dtype, write_x1=True, p=0.0, seed=0, stream_y=0, stream_out=0,
                    out_drop=False, x1=None, step=None):
    _dev(x0, y, w)
    rows, cols = x0.shape
    if x1 is None and write_x1:
        x1 = torch.empty_like(x0)
    xn = torch.empty(rows, cols, device=x0.device, dtype=xn_dtype)
    rstd = torch.empty(rows, device=x0.device, dtype=torch.float32)
    _check(load().mrmt3_add_rmsnorm_fwd(_p(x0), _p(y), _dt(y) if y is not None else F32, _p(w), eps, _p(x1), _p(xn),
                                        _dt(xn), _p(rstd), rows, cols, p, seed, _p(step), stream_y, stream_out,
                                        int(out_drop), _stream()), "add_rmsnorm_fwd")
    return (x1 if x1 is not None else x0), xn, rstd


class NormDwBatch:
    """Norm-weight gradients of one backward pass, summed in ONE launch instead of one per norm site.

    `add_rmsnorm_bwd(..., defer=batch)` leaves the site's per-workgroup partial rows in a workspace that belongs to
    (batch, dw vector, shape) and queues the site; `flush()` runs `mrmt3_norm_dw_reduce` over everything queued
    (same summation order as the immediate form, so the result is bit-identical).  The caller must flush before the
    gradients are read (the engine does so before a gradient bucket is sent and at the end of backward).  The address
    tables live on the device and are rebuilt only when the set of queued sites changes."""

    def __init__(self):
        self._ws = {}          # (dw address, rows, cols) -> workspace tensor
        self._queue = []       # [(key, dw tensor)]
        self._tables = {}      # tuple(keys) -> (ws addresses, dw addresses, partial rows) device tensors

    def site(self, dw, rows, cols, n_part=None):
        """`n_part`: partial rows the producing kernel leaves (default: the stand-alone norm backward's count)."""
        if n_part is None:
            n_part = load().mrmt3_add_rmsnorm_bwd_partial_rows(rows)
        key = (dw.data_ptr(), rows, cols, n_part)
        ws = self._ws.get(key)
        if ws is None:
            ws = torch.empty(load().mrmt3_add_rmsnorm_bwd_workspace_bytes(rows, cols), device=dw.device, dtype=torch.uint8)
            self._ws[key] = ws
        self._queue.append((key, dw))
        return ws

    def clear(self):
        """Forget the queued sites without reducing them (their partial rows were never written); workspaces and tables stay."""
        self._queue.clear()

    def flush(self):
        if not self._queue:
            return
        for cols in sorted({k[2] for k, _ in self._queue}):
            keys = tuple(k for k, _ in self._queue if k[2] == cols)
            tab = self._tables.get(keys)
            dev = self._queue[0][1].device
            if tab is None:
                tab = (torch.tensor([self._ws[k].data_ptr() for k in keys], dtype=torch.int64, device=dev),
                       torch.tensor([k[0] for k in keys], dtype=torch.int64, device=dev),
                       torch.tensor([k[3] for k in keys], dtype=torch.int32, device=dev))
                self._tables[keys] = tab
            _check(load().mrmt3_norm_dw_reduce(_p(tab[0]), _p(tab[1]), _p(tab[2]), len(keys), cols, _stream()),
                   "norm_dw_reduce")
        self._queue.clear()


def add_rmsnorm_bwd(dxn, dres, x1, rstd, w, dw, want_dy=True, p=0.0, seed=0, stream_y=0, stream_out=0,
                    out_drop=False, dx1=None, dx1_dtype=torch.float32, defer=None, step=None):
    """`dres` and the returned dx1 may be f32 or bf16 (the bf16 engine's residual-gradient stream); `dx1=`
    reuses a buffer (in place when it is `dres` itself).  `defer=` a NormDwBatch: dw is produced by its flush()."""
    _dev(dxn, x1, rstd, w)
    rows, cols = x1.shape
    if dx1 is None:
        dx1 = torch.empty(rows, cols, device=x1.device, dtype=dx1_dtype)
    dy = torch.empty(rows, cols, device=x1.device, dtype=torch.bfloat16) if want_dy else None
    if dw is None:
        ws = None
    elif defer is not None:
        ws, dw = defer.site(dw, rows, cols), None
    else:
        ws = workspace(load().mrmt3_add_rmsnorm_bwd_workspace_bytes(rows, cols), x1.device)
    _check(load().mrmt3_add_rmsnorm_bwd(_p(dxn), _dt(dxn), _p(dres), _dt(dres) if dres is not None else F32, _p(x1),
                                        _p(rstd), _p(w), _p(dx1), _dt(dx1), _p(dy), _p(dw), rows, cols, p, seed,
                                        _p(step), stream_y, stream_out, int(out_drop), _p(ws), ws.numel() if ws is not None else 0,
                                        _stream()),
           "add_rmsnorm_bwd")
    return dx1, dy


def _attn_executed_pairs(Lq, Lk, causal):
    """(query, key) pairs the flash kernels visit: 128-query tiles x 64-key tiles, causal tiles above the diagonal skipped."""
    if not causal:
        return float(Lq) * Lk
    n = 0
    for q0 in range(0, Lq, 128):
        n_kv = min(-(-Lk // 64), min(q0 + 127, Lq - 1) // 64 + 1)
        n += min(128, Lq - q0) * min(Lk, n_kv * 64)
    return float(n)


def attn_fwd(q, k, v, B, H, Lq, Lk, causal, p=0.0, seed=0, stream_id=0, want_lse=True, step=None, want_lo=None, out=None,
             out_lo=None):
    """q: [B*Lq, ldq-view], k/v: [B*Lk, ld-view] 2-D views whose column 0 is head 0 / dim 0.
    want_lo (True / False instead of None): returns (o, lse, o_lo) with o_lo = bf16(O - bf16(O)) for the backward's
    delta when True (and the kernel is the bf16 one), else None.  out / out_lo: caller-owned [B*Lq, H*64] views of the same
    row stride (a multiple of 4 elements; rows that are not 16-byte aligned take the kernel's 8-byte store path)."""
    _dev(q, k, v)
    o = torch.empty(B * Lq, H * 64, device=q.device, dtype=q.dtype) if out is None else out
    assert o.shape == (B * Lq, H * 64) and o.dtype == q.dtype and o.stride(1) == 1
    if out_lo is not None:
        assert want_lo and out_lo.shape == o.shape and out_lo.stride(0) == o.stride(0) and out_lo.dtype == o.dtype
    o_lo = (out_lo if out_lo is not None else torch.empty_like(o)) if want_lo and q.dtype == torch.bfloat16 else None
    assert o_lo is None or o_lo.stride(0) == o.stride(0)
    lse = torch.empty(B, H, Lq, device=q.device, dtype=torch.float32) if want_lse else None
    # algorithmic FLOPs count the full (unskipped) square, as the reference computes it
    with _Timed("attn_fwd", 4.0 * B * H * Lq * Lk * 64, "FLOP", executed=4.0 * B * H * 64 * _attn_executed_pairs(Lq, Lk, causal)):
        _check(load().mrmt3_attn_fwd(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), o.stride(0),
                                     _p(o_lo), _p(lse), B, H, Lq, Lk, int(causal), _dt(q), p, seed, _p(step), stream_id,
                                     _stream()),
               "attn_fwd")
    if want_lo is not None:
        return o, lse, o_lo
    return o, lse


def attn_bwd(q, k, v, o, d_o, lse, dq, dk, dv, B, H, Lq, Lk, causal, p=0.0, seed=0, stream_id=0, step=None, o_lo=None):
    _dev(q, k, v, o, d_o, lse, dq, dk, dv, o_lo)
    assert o_lo is None or (o_lo.shape == o.shape and o_lo.stride(0) == o.stride(0))
    delta = torch.empty(B, H, Lq, device=q.device, dtype=torch.float32)
    if q.dtype == torch.float32:                     # exact-f32 path (fp32 training / parity)
        assert all(t.dtype == torch.float32 for t in (k, v, o, d_o, dq, dk, dv))
        _check(load().mrmt3_attn_bwd_f32(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), o.stride(0),
                                         _p(d_o), d_o.stride(0), _p(lse), _p(delta), _p(dq), dq.stride(0), _p(dk),
                                         dk.stride(0), _p(dv), dv.stride(0), B, H, Lq, Lk, int(causal), p, seed,
                                         _p(step), stream_id, _stream()), "attn_bwd_f32")
        return dq, dk, dv
    with _Timed("attn_bwd", 8.0 * B * H * Lq * Lk * 64, "FLOP", executed=8.0 * B * H * 64 * _attn_executed_pairs(Lq, Lk, causal)):
        _check(load().mrmt3_attn_bwd(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), o.stride(0),
                                     _p(o_lo), _p(d_o), d_o.stride(0), _p(lse), _p(delta), _p(dq), dq.stride(0), _p(dk),
                                     dk.stride(0), _p(dv), dv.stride(0), B, H, Lq, Lk, int(causal), p, seed,
                                     _p(step), stream_id, _stream()), "attn_bwd")
    return dq, dk, dv


class PackPlan:
    """Device tensors of one packed batch (mrmt3_pack_plan, csrc/pack.hip): row b of the [B, L] labels owns packed rows
    [row_off[b], row_off[b+1]) of Tcap."""

    def __init__(self, B, L, Tcap, device):
        i32 = dict(device=device, dtype=torch.int32)
        self.B, self.L, self.Tcap = B, L, Tcap
        self.n_ent = load().mrmt3_pack_tile_entries(B, Tcap)
        self.len = torch.empty(B, **i32)
        self.row_off = torch.empty(B + 1, **i32)
        self.tok_row = torch.empty(Tcap, **i32)
        self.tok_pos = torch.empty(Tcap, **i32)
        self.dec_ids = torch.empty(Tcap, device=device, dtype=torch.int64)
        self.targets = torch.empty(Tcap, device=device, dtype=torch.int64)
        self.tiles = torch.empty(2 + 2 * self.n_ent, **i32)
        self.err = torch.empty(1, **i32)


def pack_lengths(labels):
    """len [B] int32 on the device: 1 + the last position of each row whose label is not -100 (0 for none)."""
    _dev(labels)
    assert labels.dtype == torch.int64 and labels.dim() == 2 and labels.is_contiguous()
    B, L = labels.shape
    out = torch.empty(B, device=labels.device, dtype=torch.int32)
    _check(load().mrmt3_pack_lengths(_p(labels), B, L, _p(out), _stream()), "pack_lengths")
    return out


def pack_plan(labels, Tcap, start_id, pad_id, plan=None):
    """The packing plan of labels [B, L] int64 (device) at capacity Tcap: a PackPlan (its `err` is 1 when the rows do not fit)."""
    _dev(labels)
    assert labels.dtype == torch.int64 and labels.dim() == 2 and labels.is_contiguous()
    B, L = labels.shape
    pl = plan if plan is not None else PackPlan(B, L, Tcap, labels.device)
    _check(load().mrmt3_pack_plan(_p(labels), B, L, Tcap, start_id, pad_id, _p(pl.len), _p(pl.row_off), _p(pl.tok_row),
                                  _p(pl.tok_pos), _p(pl.dec_ids), _p(pl.targets), _p(pl.tiles), _p(pl.err), _stream()),
           "pack_plan")
    return pl


def embed_fwd_packed(plan, table, pos, p=0.0, seed=0, stream_id=0, step=None):
    """Embedding of the packed decoder inputs: table[dec_ids] + pos[tok_pos], dropout keyed by the packed row.  [Tcap, d] f32."""
    _dev(table, pos)
    V, d = table.shape
    x = torch.empty(plan.Tcap, d, device=table.device, dtype=torch.float32)
    _check(load().mrmt3_embed_fwd_packed(_p(plan.dec_ids), _p(plan.tok_pos), _p(table), _p(pos), _p(x), plan.Tcap, d, V, p, seed,
                                         _p(step), stream_id, _stream()), "embed_fwd_packed")
    return x


def packed_attn_pairs(lengths, Lk, causal):
    """(query, key) pairs of a packed launch from the host-side row lengths: the algorithmic work of the varlen kernels."""
    if Lk:
        return float(sum(lengths)) * Lk
    if causal:
        return float(sum(n * (n + 1) // 2 for n in lengths))
    return float(sum(n * n for n in lengths))


def attn_fwd_varlen(q, k, v, plan, H, Lk, causal, p=0.0, seed=0, stream_id=0, step=None, want_lse=True, want_lo=False,
                    lengths=None):
    """Attention over packed rows: q [Tcap, *] (head h at columns h*64..), k / v packed like q (Lk = 0, self-attention) or dense
    [B*Lk, *] (cross-attention).  Returns (o [Tcap, H*64], lse [H, Tcap] or None, o_lo or None).  `lengths` (host list, optional)
    only prices the launch for the profile."""
    _dev(q, k, v)
    T = plan.Tcap
    assert q.shape[0] == T and (k.shape[0] == (T if Lk == 0 else plan.B * Lk))
    o = torch.empty(T, H * 64, device=q.device, dtype=q.dtype)
    o_lo = torch.empty_like(o) if want_lo and q.dtype == torch.bfloat16 else None
    lse = torch.empty(H, T, device=q.device, dtype=torch.float32) if want_lse else None
    work = 4.0 * H * 64 * packed_attn_pairs(lengths, Lk, causal) if lengths is not None else 0.0
    with _Timed("attn_fwd_varlen", work, "FLOP"):
        _check(load().mrmt3_attn_fwd_varlen(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), o.stride(0),
                                            _p(o_lo), _p(lse), _p(plan.row_off), _p(plan.tiles), plan.B, H, T, plan.L, Lk,
                                            int(causal), _dt(q), p, seed, _p(step), stream_id, _stream()), "attn_fwd_varlen")
    return o, lse, o_lo


def attn_bwd_varlen(q, k, v, o, d_o, lse, dq, dk, dv, plan, H, Lk, causal, p=0.0, seed=0, stream_id=0, step=None, o_lo=None,
                    lengths=None):
    """Backward of attn_fwd_varlen into caller-owned dq (packed like q) and dk / dv (laid out like k / v)."""
    _dev(q, k, v, o, d_o, lse, dq, dk, dv, o_lo)
    delta = torch.empty(H, plan.Tcap, device=q.device, dtype=torch.float32)
    work = 8.0 * H * 64 * packed_attn_pairs(lengths, Lk, causal) if lengths is not None else 0.0
    with _Timed("attn_bwd_varlen", work, "FLOP"):
        _check(load().mrmt3_attn_bwd_varlen(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), o.stride(0),
                                            _p(o_lo), _p(d_o), d_o.stride(0), _p(lse), _p(delta), _p(dq), dq.stride(0), _p(dk),
                                            dk.stride(0), _p(dv), dv.stride(0), _p(plan.row_off), _p(plan.tiles), plan.B, H,
                                            plan.Tcap, plan.L, Lk, int(causal), _dt(q), p, seed, _p(step), stream_id,
                                            _stream()), "attn_bwd_varlen")
    return dq, dk, dv


def _bias_stride(bias, B, H, Lq, Lk):
    assert bias.dtype == torch.float32 and bias.is_contiguous()
    if tuple(bias.shape) == (H, Lq, Lk):
        return 0
    assert tuple(bias.shape) == (B, H, Lq, Lk), "bias is [H, Lq, Lk] (shared by the batch) or [B, H, Lq, Lk]"
    return H * Lq * Lk


def attn_fwd_bias(q, k, v, bias, B, H, Lq, Lk, causal, p=0.0, seed=0, stream_id=0, step=None):
    """softmax(q k^T + bias [+ causal]) v — HF T5Attention with its additive position bias (models/t5.py:636-648).  The
    general kernel (f32 arithmetic on f32 / bf16 operands), not the MFMA path: MR-MT3's own bias is zero and its step
    calls attn_fwd.  Returns (o, lse)."""
    _dev(q, k, v, bias)
    o = torch.empty(B * Lq, H * 64, device=q.device, dtype=q.dtype)
    lse = torch.empty(B, H, Lq, device=q.device, dtype=torch.float32)
    bs = 0 if bias is None else _bias_stride(bias, B, H, Lq, Lk)
    _check(load().mrmt3_attn_fwd_bias(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(bias), bs, _p(o),
                                      o.stride(0), _p(lse), B, H, Lq, Lk, int(causal), _dt(q), p, seed, _p(step), stream_id,
                                      _stream()), "attn_fwd_bias")
    return o, lse


def attn_bwd_bias(q, k, v, o, d_o, lse, bias, B, H, Lq, Lk, causal, p=0.0, seed=0, stream_id=0, step=None, want_dbias=True):
    """Backward of attn_fwd_bias: returns (dq, dk, dv, dbias); dbias has the bias's shape (summed over the batch when the
    bias is shared) or is None."""
    _dev(q, k, v, o, d_o, lse, bias)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    delta = torch.empty(B, H, Lq, device=q.device, dtype=torch.float32)
    bs = 0 if bias is None else _bias_stride(bias, B, H, Lq, Lk)
    dbias = torch.empty_like(bias) if (want_dbias and bias is not None) else None
    _check(load().mrmt3_attn_bwd_bias(_p(q), q.stride(0), _p(k), k.stride(0), _p(v), v.stride(0), _p(o), o.stride(0),
                                      _p(d_o), d_o.stride(0), _p(lse), _p(delta), _p(bias), bs, _p(dq), dq.stride(0), _p(dk),
                                      dk.stride(0), _p(dv), dv.stride(0), _p(dbias), B, H, Lq, Lk, int(causal), _dt(q), p,
                                      seed, _p(step), stream_id, _stream()), "attn_bwd_bias")
    return dq, dk, dv, dbias


def geglu_fwd(h, p=0.0, seed=0, stream_id=0, step=None):
    _dev(h)
    rows, two = h.shape
    g = torch.empty(rows, two // 2, device=h.device, dtype=h.dtype)
    _check(load().mrmt3_geglu_fwd(_p(h), _p(g), rows, two // 2, _dt(h), p, seed, _p(step), stream_id, _stream()),
           "geglu_fwd")
    return g


def gemm_nt_geglu(x, wi, p=0.0, seed=0, stream_id=0, step=None):
    """h = x . wi^T and g = dropout(gelu_new(h0) * h1) in one launch (bf16); returns (h, g), bit-identical to
    gemm_nt + geglu_fwd."""
    assert x.dtype == torch.bfloat16 and wi.dtype == torch.bfloat16 and x.stride(-1) == 1 and wi.stride(-1) == 1
    rows, K = x.shape
    two = wi.shape[0]
    h = torch.empty(rows, two, device=x.device, dtype=torch.bfloat16)
    g = torch.empty(rows, two // 2, device=x.device, dtype=torch.bfloat16)
    with _Timed("gemm_nt_geglu_bf16", 2.0 * rows * two * K, "FLOP"):      # (its own family: GEMM + gated-GELU epilogue)
        _check(load().mrmt3_gemm_nt_geglu(_p(x), x.stride(0), _p(wi), wi.stride(0), _p(h), two, _p(g), two // 2, rows,
                                          two // 2, K, p, seed, _p(step), stream_id, _stream()), "gemm_nt_geglu")
    return h, g


def gemm_rows_ok(a, w, N=512):
    """True when the fused projection + row kernels (gemm_rows.hip) take a [M, K] x [N, K]^T product of these operands."""
    return (a.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and a.dim() == 2 and w.dim() == 2 and
            a.stride(1) == 1 and w.stride(1) == 1 and w.shape[0] == N and a.shape[1] == w.shape[1] and
            bool(load().mrmt3_gemm_rows_ok(a.shape[0], N, a.shape[1], a.stride(0), w.stride(0))))


def _rows_bytes(M, N, K, row_bytes):
    """algorithmic bytes of a fused launch: operands once + `row_bytes` per output element of the row operands"""
    return (M * K + N * K) * 2 + M * N * row_bytes


def gemm_nt_addnorm(a, w_proj, x0, w_norm, eps, write_x1=True, p=0.0, seed=0, stream_y=0, stream_out=0, out_drop=False,
                    x1=None, step=None):
    """(x1, xn, rstd) = add_rmsnorm_fwd(x0, gemm_nt(a, w_proj), w_norm, ...) in ONE launch (bf16; same bits)."""
    _dev(a, w_proj, x0, w_norm)
    rows, K = a.shape
    assert x0.shape == (rows, 512) and x0.dtype == torch.float32 and x0.is_contiguous()
    if x1 is None and write_x1:
        x1 = torch.empty_like(x0)
    xn = torch.empty(rows, 512, device=a.device, dtype=torch.bfloat16)
    rstd = torch.empty(rows, device=a.device, dtype=torch.float32)
    if PROFILE is not None:
        PROFILE_BYTES["gemm_nt_addnorm_bf16"] = PROFILE_BYTES.get("gemm_nt_addnorm_bf16", 0.0) + _rows_bytes(rows, 512, K, 10)
    with _Timed("gemm_nt_addnorm_bf16", 2.0 * rows * 512 * K, "FLOP"):
        _check(load().mrmt3_gemm_nt_addnorm(_p(a), a.stride(0), _p(w_proj), w_proj.stride(0), rows, K, _p(x0), _p(w_norm),
                                            eps, _p(x1), _p(xn), _p(rstd), p, seed, _p(step), stream_y, stream_out,
                                            int(out_drop), _stream()), "gemm_nt_addnorm")
    return (x1 if x1 is not None else x0), xn, rstd


def gemm_nt_normbwd(a, wt, dres, x1, rstd, w_norm, dw, want_dy=True, p=0.0, seed=0, stream_y=0, dx1=None,
                    dx1_dtype=torch.float32, defer=None, step=None):
    """(dx1, dy) = add_rmsnorm_bwd(gemm_nt(a, wt), dres, x1, rstd, w_norm, dw, ...) in ONE launch (bf16 product)."""
    _dev(a, wt, dres, x1, rstd, w_norm)
    rows, K = a.shape
    assert x1.shape == (rows, 512) and dres is not None and dres.shape == (rows, 512)
    if dx1 is None:
        dx1 = torch.empty(rows, 512, device=a.device, dtype=dx1_dtype)
    dy = torch.empty(rows, 512, device=a.device, dtype=torch.bfloat16) if want_dy else None
    L = load()
    n_part = L.mrmt3_gemm_nt_normbwd_partial_rows(rows)
    reduce_now = None
    if dw is None:
        ws = None
    elif defer is not None:
        ws = defer.site(dw, rows, 512, n_part)
    else:
        ws = workspace(L.mrmt3_add_rmsnorm_bwd_workspace_bytes(rows, 512), a.device)
        reduce_now = dw
    if PROFILE is not None:
        PROFILE_BYTES["gemm_nt_normbwd_bf16"] = PROFILE_BYTES.get("gemm_nt_normbwd_bf16", 0.0) + _rows_bytes(
            rows, 512, K, 4 + dres.element_size() + dx1.element_size() + (2 if want_dy else 0))
    with _Timed("gemm_nt_normbwd_bf16", 2.0 * rows * 512 * K, "FLOP"):
        _check(L.mrmt3_gemm_nt_normbwd(_p(a), a.stride(0), _p(wt), wt.stride(0), rows, K, _p(dres), _dt(dres), _p(x1),
                                       _p(rstd), _p(w_norm), _p(dx1), _dt(dx1), _p(dy), p, seed, _p(step), stream_y,
                                       _p(ws), ws.numel() if ws is not None else 0, _stream()), "gemm_nt_normbwd")
    if reduce_now is not None:
        # the one-site address table of the reduce, cached per (workspace, dw, partial rows): built by a synchronous
        # host-to-device copy, which a hipGraph capture of the step does not allow — the eager warm-up steps leave it here
        key = (ws.data_ptr(), dw.data_ptr(), n_part, a.device.index)
        tab = _NORMBWD_TABLES.get(key)
        if tab is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("gemm_nt_normbwd: the norm-weight reduce table of this site was not prepared before the "
                                   "capture (run the step eagerly once with the same buffers, or pass defer=NormDwBatch)")
            dev = a.device
            tab = _NORMBWD_TABLES[key] = (torch.tensor([ws.data_ptr()], dtype=torch.int64, device=dev),
                                          torch.tensor([dw.data_ptr()], dtype=torch.int64, device=dev),
                                          torch.tensor([n_part], dtype=torch.int32, device=dev))
            if len(_NORMBWD_TABLES) > 256:
                _NORMBWD_TABLES.pop(next(iter(_NORMBWD_TABLES)))
        _check(L.mrmt3_norm_dw_reduce(_p(tab[0]), _p(tab[1]), _p(tab[2]), 1, 512, _stream()), "norm_dw_reduce")
    return dx1, dy


_NORMBWD_TABLES = {}


def gemm_nt_geglubwd(dy, wt, h, p=0.0, seed=0, stream_id=0, step=None):
    """dh = geglu_bwd(h, gemm_nt(dy, wt)) in ONE launch (wt = wo^T [dff, d]; bf16; same bits)."""
    _dev(dy, wt, h)
    rows, K = dy.shape
    dff = wt.shape[0]
    assert h.shape == (rows, 2 * dff) and h.dtype == torch.bfloat16 and h.is_contiguous()
    dh = torch.empty_like(h)
    if PROFILE is not None:
        PROFILE_BYTES["gemm_nt_geglubwd_bf16"] = PROFILE_BYTES.get("gemm_nt_geglubwd_bf16", 0.0) + _rows_bytes(rows, dff, K, 8)
    with _Timed("gemm_nt_geglubwd_bf16", 2.0 * rows * dff * K, "FLOP"):
        _check(load().mrmt3_gemm_nt_geglubwd(_p(dy), dy.stride(0), _p(wt), wt.stride(0), _p(h), _p(dh), rows, dff, K, p,
                                             seed, _p(step), stream_id, _stream()), "gemm_nt_geglubwd")
    return dh


def geglu_bwd(h, dg, p=0.0, seed=0, stream_id=0, step=None):
    _dev(h, dg)
    rows, two = h.shape
    dh = torch.empty_like(h)
    assert dg.dtype == h.dtype
    _check(load().mrmt3_geglu_bwd(_p(h), _p(dg), _p(dh), rows, two // 2, _dt(h), p, seed, _p(step), stream_id, _stream()),
           "geglu_bwd")
    return dh


def embed_fwd(ids, table, pos, seq_len, shift, start_id=0, pad_id=0, pos_offset=0, p=0.0, seed=0, stream_id=0,
              step=None):
    _dev(ids, table, pos)
    rows = ids.numel()
    V, d = table.shape
    x = torch.empty(rows, d, device=table.device, dtype=torch.float32)
    _check(load().mrmt3_embed_fwd(_p(ids), _p(table), _p(pos), _p(x), rows, seq_len, d, V, int(shift), start_id,
                                  pad_id, pos_offset, p, seed, _p(step), stream_id, _stream()), "embed_fwd")
    return x


def embed_bwd(ids, dx, dtable, seq_len, shift, start_id=0, pad_id=0, p=0.0, seed=0, stream_id=0, step=None):
    _dev(ids, dx, dtable)
    rows = ids.numel()
    V, d = dtable.shape
    ws = workspace(load().mrmt3_embed_bwd_workspace_bytes(rows, V, d), dx.device)
    _check(load().mrmt3_embed_bwd(_p(ids), _p(dx), _p(dtable), rows, seq_len, d, V, int(shift), start_id, pad_id, p,
                                  seed, _p(step), stream_id, _p(ws), ws.numel(), _stream()), "embed_bwd")


def addpos_fwd(src, pos, seq_len, pos_offset=0, p=0.0, seed=0, stream_id=0, step=None):
    _dev(src, pos)
    rows, d = src.shape
    x = torch.empty(rows, d, device=src.device, dtype=torch.float32)
    _check(load().mrmt3_addpos_fwd(_p(src), _dt(src), _p(pos), _p(x), rows, seq_len, d, pos_offset, p, seed,
                                   _p(step), stream_id, _stream()), "addpos_fwd")
    return x


def dropmask_cast(dx, p=0.0, seed=0, stream_id=0, step=None, out_dtype=torch.bfloat16):
    _dev(dx)
    out = torch.empty(dx.shape, device=dx.device, dtype=out_dtype)
    _check(load().mrmt3_dropmask_cast(_p(dx), _p(out), _dt(out), dx.numel(), p, seed, _p(step), stream_id, _stream()),
           "dropmask_cast")
    return out


def ce_options(label_smoothing=0.0, z_loss=0.0):
    """Validate the loss options (host only) -> (on, label_smoothing, z_loss) as floats: 0 <= label_smoothing < 1 (the
    keyword of torch.nn.CrossEntropyLoss), z_loss >= 0 and finite (T5X's z_loss); `on` iff either is non-zero."""
    out = []
    for name, val in (("label_smoothing", label_smoothing), ("z_loss", z_loss)):
        if isinstance(val, bool) or not isinstance(val, (int, float)):
            raise ValueError("%s must be a number, got %r" % (name, val))
        out.append(float(val))
    eps, z = out
    if not 0.0 <= eps < 1.0:
        raise ValueError("label_smoothing must be in [0, 1), got %r" % (label_smoothing,))
    if not 0.0 <= z < float("inf"):
        raise ValueError("z_loss must be finite and >= 0, got %r" % (z_loss,))
    return (eps != 0.0 or z != 0.0), eps, z


def cross_entropy(logits, targets, want_grad=True, grad_dtype=torch.bfloat16, weighted=False, inst_lo=1135,
                  inst_hi=1262, grad_scale=1.0, label_smoothing=0.0, z_loss=0.0, return_nll=False):
    """Returns (loss_dev[1] f32 tensor, dlogits or None).  No host sync.  With label_smoothing / z_loss the
    first element is the regularised objective, whose gradient dlogits is; `return_nll=True` appends the plain NLL (with
    both options off the loss itself, from the unchanged mrmt3_ce_fwd_bwd)."""
    reg, eps, z = ce_options(label_smoothing, z_loss)
    _dev(logits, targets)
    rows, V = logits.shape
    # [loss (double accumulator), denom (f32 in its first 4 bytes)]; with the options on [objective, nll, denom]
    acc = torch.zeros(3 if reg else 2, device=logits.device, dtype=torch.float64)
    den = C.c_void_p(acc.data_ptr() + (16 if reg else 8))
    lib = load()
    _check(lib.mrmt3_ce_count(_p(targets), rows, int(weighted), inst_lo, inst_hi, den, _stream()), "ce_count")
    dl = torch.empty(rows, V, device=logits.device, dtype=grad_dtype) if want_grad else None
    if reg:
        _check(lib.mrmt3_ce_fwd_bwd_reg(_p(logits), _p(targets), den, eps, z, _p(acc), _p(dl),
                                        _dt(dl) if dl is not None else F32, rows, V, int(weighted), inst_lo, inst_hi,
                                        grad_scale, _stream()), "ce_fwd_bwd_reg")
        both = acc[0:2].float()
        return (both[0:1], dl, both[1:2]) if return_nll else (both[0:1], dl)
    _check(lib.mrmt3_ce_fwd_bwd(_p(logits), _p(targets), den, _p(acc), _p(dl),
                                _dt(dl) if dl is not None else F32, rows, V, int(weighted), inst_lo, inst_hi,
                                grad_scale, _stream()), "ce_fwd_bwd")
    loss = acc[0:1].float()
    return (loss, dl, loss) if return_nll else (loss, dl)


def ce_chunk_rows() -> int:
    """MRMT3_CE_CHUNK (rows of logits per lm_head + CE chunk), validated: an integer, at least 1024."""
    raw = os.environ.get("MRMT3_CE_CHUNK", "65536")
    try:
        n = int(raw)
    except ValueError:
        raise ValueError(f"MRMT3_CE_CHUNK={raw!r} is not an integer") from None
    if n < 1024:
        raise ValueError(f"MRMT3_CE_CHUNK={n}: a chunk is at least 1024 rows")
    return n


def lmhead_cross_entropy(dec, w, targets, want_grad=True, grad_dtype=torch.bfloat16, weighted=False, inst_lo=1135,
                         inst_hi=1262, grad_scale=1.0, chunk_rows=None, label_smoothing=0.0, z_loss=0.0, return_nll=False):
    """lm_head + CE fused over row chunks (mrmt3_lmhead_ce_fwd_bwd): dec [rows, d] bf16, w [V, d] bf16 ->
    (loss_dev[1] f32, dlogits [rows, V] or None).  The f32 logits only ever exist one chunk at a time, in a workspace.
    label_smoothing / z_loss / return_nll as for cross_entropy (mrmt3_lmhead_ce_fwd_bwd_reg when either option is on)."""
    reg, eps, z = ce_options(label_smoothing, z_loss)
    _dev(dec, w, targets)
    rows, d = dec.shape
    V = w.shape[0]
    assert dec.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and dec.stride(1) == 1 and w.stride(1) == 1
    if chunk_rows is None:
        # 65 536 rows = 403 MB of f32 logits in the workspace: the 64-segment step in ONE chunk (25.41 -> 25.32 ms against
        # four chunks of 16 384, same box); larger batches still go chunk by chunk (MRMT3_CE_CHUNK)
        chunk_rows = ce_chunk_rows()
    # [loss (double accumulator), denom (f32 in its first 4 bytes)]; with the options on [objective, nll, denom]
    acc = torch.zeros(3 if reg else 2, device=dec.device, dtype=torch.float64)
    den = C.c_void_p(acc.data_ptr() + (16 if reg else 8))
    lib = load()
    _check(lib.mrmt3_ce_count(_p(targets), rows, int(weighted), inst_lo, inst_hi, den, _stream()), "ce_count")
    dl = torch.empty(rows, V, device=dec.device, dtype=grad_dtype) if want_grad else None
    ws = workspace(min(rows, chunk_rows) * V * 4, dec.device)
    if reg:
        _check(lib.mrmt3_lmhead_ce_fwd_bwd_reg(_p(dec), dec.stride(0), _p(w), w.stride(0), _p(targets), den, eps, z,
                                               _p(acc), _p(dl), _dt(dl) if dl is not None else F32,
                                               rows, V, d, int(weighted), inst_lo, inst_hi, grad_scale, _p(ws), ws.numel(),
                                               chunk_rows, _stream()), "lmhead_ce_fwd_bwd_reg")
        both = acc[0:2].float()
        return (both[0:1], dl, both[1:2]) if return_nll else (both[0:1], dl)
    _check(lib.mrmt3_lmhead_ce_fwd_bwd(_p(dec), dec.stride(0), _p(w), w.stride(0), _p(targets),
                                       den, _p(acc), _p(dl), _dt(dl) if dl is not None else F32,
                                       rows, V, d, int(weighted), inst_lo, inst_hi, grad_scale, _p(ws), ws.numel(),
                                       chunk_rows, _stream()), "lmhead_ce_fwd_bwd")
    loss = acc[0:1].float()
    return (loss, dl, loss) if return_nll else (loss, dl)


def token_logprob(logits, targets, ignore_index=-100):
    """out[r] = log_softmax(logits[r])[targets[r]] (f32), 0 where the target is `ignore_index` (mrmt3_token_logprob)."""
    _dev(logits, targets)
    rows, V = logits.shape
    assert logits.dtype == torch.float32 and logits.is_contiguous()
    assert targets.dtype == torch.int64 and targets.is_contiguous() and targets.numel() == rows
    out = torch.empty(rows, device=logits.device, dtype=torch.float32)
    _check(load().mrmt3_token_logprob(_p(logits), _p(targets), _p(out), rows, V, int(ignore_index), _stream()),
           "token_logprob")
    return out


def sample_logits(logits, temperature=1.0, top_k=0, top_p=1.0, seed=0, step=0, row0=0, ban=None, return_logprobs=False):
    """One draw per row of [rows, V] f32 logits by the decoder's sampling rule (mrmt3_sample_logits): row r
    uses the counter (row0 + r, step).  `ban`: device [V] uint8 mask or None.  -> tokens [rows] int64, and with
    `return_logprobs` the log-probability of each under the softmax of the logits after the ban."""
    _dev(logits)
    rows, V = logits.shape
    assert logits.dtype == torch.float32 and logits.is_contiguous()
    assert ban is None or (ban.dtype == torch.uint8 and ban.is_contiguous() and ban.numel() == V and ban.is_cuda)
    tok = torch.empty(rows, device=logits.device, dtype=torch.int64)
    lp = torch.empty(rows, device=logits.device, dtype=torch.float32) if return_logprobs else None
    _check(load().mrmt3_sample_logits(_p(logits), rows, V, _p(ban), float(temperature), int(top_k), float(top_p), int(seed),
                                      int(step), int(row0), _p(tok), _p(lp), _stream()), "sample_logits")
    return (tok, lp) if return_logprobs else tok


class GrammarState:
    """A stand-alone grammar state on the device (mrmt3_grammar_init / _advance / _active): `rows` event-grammar
    state machines and their [rows, V] uint8 masks (1 = the row may not emit that token next).  The decoder keeps one of its
    own inside the captured step; this is the same device code on its own, for tests and tools."""

    def __init__(self, grammar, rows, V, device, carry=None, ban=None):
        assert carry is None or (carry.dtype == torch.uint8 and carry.is_contiguous() and carry.is_cuda
                                 and tuple(carry.shape) == (rows, 2048))
        assert ban is None or (ban.dtype == torch.uint8 and ban.is_contiguous() and ban.numel() == V and ban.is_cuda)
        self.grammar, self.rows, self.V = grammar, rows, V
        self._g = grammar.c_struct()
        self._keep = (carry, ban)          # the state keeps both pointers
        self.state = torch.zeros(int(load().mrmt3_grammar_state_bytes(rows)), dtype=torch.uint8, device=device)
        self.mask = torch.empty(rows, V, dtype=torch.uint8, device=device)
        _check(load().mrmt3_grammar_init(C.byref(self._g), _p(self.state), _p(carry), _p(ban), rows, V, _p(self.mask),
                                         _stream()), "grammar_init")

    def advance(self, tokens, parents=None):
        """Row r takes row parents[r]'s state (its own without `parents`), pushes tokens[r]; -> the new masks (a view)."""
        assert tokens.dtype == torch.int64 and tokens.is_contiguous() and tokens.numel() == self.rows and tokens.is_cuda
        assert parents is None or (parents.dtype == torch.int32 and parents.is_contiguous() and parents.numel() == self.rows
                                   and parents.is_cuda)
        _check(load().mrmt3_grammar_advance(C.byref(self._g), _p(self.state), _p(parents), _p(tokens), self.rows, self.V,
                                            _p(self.mask), _stream()), "grammar_advance")
        return self.mask

    def active(self):
        """[rows, 2048] uint8: every row's `active` bit set (bit program * 128 + pitch)."""
        out = torch.empty(self.rows, 2048, dtype=torch.uint8, device=self.state.device)
        _check(load().mrmt3_grammar_active(_p(self.state), self.rows, _p(out), _stream()), "grammar_active")
        return out


def grammar_replay(grammar, ids, V, carry=None):
    """[rows, 2048] uint8: the `active` set each row of `ids` [rows, W] int64 (start token first) leaves behind under
    `grammar`, from `carry` [rows, 2048] or nothing (mrmt3_grammar_replay): the next segment's carry."""
    _dev(ids)
    rows, W = ids.shape
    assert ids.dtype == torch.int64 and ids.is_contiguous()
    assert carry is None or (carry.dtype == torch.uint8 and carry.is_contiguous() and carry.is_cuda
                             and tuple(carry.shape) == (rows, 2048))
    g = grammar.c_struct()
    out = torch.empty(rows, 2048, dtype=torch.uint8, device=ids.device)
    _check(load().mrmt3_grammar_replay(C.byref(g), _p(ids), W, rows, W - 1, int(V), _p(carry), _p(out), _stream()),
           "grammar_replay")
    return out


def lmhead_logprob(dec, w, targets, chunk_rows=None):
    """lm_head + log-probability of each row's target over row chunks (mrmt3_lmhead_logprob): dec [rows, d], w [V, d] of
    one dtype (bf16 or f32), targets [rows] int64 -> [rows] f32, 0 at -100.  The f32 logits exist one chunk at a time."""
    _dev(dec, w, targets)
    rows, d = dec.shape
    V = w.shape[0]
    assert dec.dtype == w.dtype and w.shape[1] == d and dec.stride(1) == 1 and w.stride(1) == 1
    assert targets.dtype == torch.int64 and targets.is_contiguous() and targets.numel() == rows
    if chunk_rows is None:
        chunk_rows = ce_chunk_rows()
    out = torch.empty(rows, device=dec.device, dtype=torch.float32)
    ws = workspace(min(rows, chunk_rows) * V * 4, dec.device)
    _check(load().mrmt3_lmhead_logprob(_p(dec), dec.stride(0), _p(w), w.stride(0), _p(targets), _p(out), rows, V, d,
                                       _dt(dec), _p(ws), ws.numel(), int(chunk_rows), _stream()), "lmhead_logprob")
    return out


class _OptRange(C.Structure):          # = mrmt3_opt_range
    _fields_ = [("begin", C.c_longlong), ("end", C.c_longlong), ("weight_decay", C.c_float), ("lr_scale", C.c_float)]


class OptRanges:
    """The table adamw_step / grad_norm read through `ranges=`: `ranges` = [(begin, end, weight_decay, lr_scale)] over a
    flat buffer of `n` elements, checked and laid out by the library's host-side planner (mrmt3_opt_ranges_plan; no GPU
    needed for that: a ValueError names what is wrong).  `to(device)` copies the table there once; the kernels read it by
    pointer, so a captured step keeps following the same table object."""

    def __init__(self, ranges, n: int):
        self.ranges = [(int(a), int(b), float(wd), float(sc)) for a, b, wd, sc in ranges]
        self.n = int(n)
        L = load()
        arr = (_OptRange * max(1, len(self.ranges)))()
        for i, r in enumerate(self.ranges):
            arr[i] = _OptRange(*r)
        nbytes = int(L.mrmt3_opt_ranges_table_bytes(len(self.ranges)))
        self.host = torch.zeros(max(nbytes, 8), dtype=torch.uint8)
        tr = C.c_size_t(0)
        rc = L.mrmt3_opt_ranges_plan(arr, len(self.ranges), self.n, C.c_void_p(self.host.data_ptr()), nbytes, C.byref(tr))
        if rc != 0:
            raise ValueError(L.mrmt3_last_error().decode())
        self.n_trainable = int(tr.value)
        self.table = None

    def __len__(self):
        return len(self.ranges)

    def to(self, device):
        if self.table is None or self.table.device != torch.device(device):
            self.table = self.host.to(device)
        return self


def adamw_step(p, g, m, v, lr_dev, step_dev, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=None, grad_scale=1.0,
               shadow=None, stat=None, clip_value=0.0, ranges: OptRanges = None, ema=None, ema_decay=0.0):
    """One AdamW step over the flat buffers; step_dev advances whatever happens.  `stat` (what grad_norm wrote): the
    gradient is g * grad_scale * stat[1], clamped to +-clip_value when > 0, and stat[2] != 0 skips the update.  `ranges`:
    only the elements of the table step, each range with its own weight decay and lr factor (everything else keeps its
    bits; `weight_decay` must then be left out), and with `ema`/`ema_decay` the EMA weights follow in the same pass.
    Without `ranges`, `weight_decay` defaults to 0.01."""
    if ranges is not None and weight_decay is not None:
        raise ValueError("adamw_step: weight_decay comes from the range table; do not pass it together with `ranges`")
    _dev(p, g, m, v, lr_dev, step_dev, stat, ema, None if ranges is None else ranges.table)
    assert stat is None or (stat.dtype == torch.float32 and stat.numel() >= 3)
    assert ranges is None or (p.dtype == torch.float32 and p.is_contiguous() and p.numel() == ranges.n)
    tab, nr, ntr = (None, 0, 0) if ranges is None else (ranges.table, len(ranges), ranges.n_trainable)
    wd = 0.01 if weight_decay is None else weight_decay
    _check(load().mrmt3_adamw_step(_p(p), _p(g), _p(m), _p(v), _p(ema), p.numel(), _p(tab), nr, ntr, _p(lr_dev),
                                   _p(step_dev), beta1, beta2, eps, wd, grad_scale, float(ema_decay), _p(stat),
                                   float(clip_value), _p(shadow), _stream()), "adamw_step")


def grad_norm_workspace(device) -> torch.Tensor:
    """The f32 workspace mrmt3_grad_norm leaves its per-workgroup f64 partials in (allocate once, outside any capture)."""
    return torch.empty(int(load().mrmt3_grad_norm_workspace_elems()), device=device, dtype=torch.float32)


def grad_norm(g, grad_scale, max_norm, skip_nonfinite, ws, stat, skipped, ranges: OptRanges = None):
    """Global L2 norm of the flat f32 gradient `g` times grad_scale, on the device, in a fixed summation order (f64
    accumulation): stat[0] = norm, stat[1] = clip coefficient min(1, max_norm / (norm + 1e-6)) (1 when max_norm is 0),
    stat[2] = 1.0 when skip_nonfinite and the norm is inf / NaN (then coef = 0 and skipped[0] += 1).  No host sync.
    `ranges`: over the elements of the table only (frozen gradient slots hold stale values and are not read)."""
    _dev(g, ws, stat, skipped, None if ranges is None else ranges.table)
    assert g.dtype == torch.float32 and g.is_contiguous() and ws.dtype == torch.float32
    assert stat.dtype == torch.float32 and stat.numel() >= 3 and skipped.dtype == torch.int32 and skipped.numel() >= 1
    assert ranges is None or g.numel() == ranges.n
    tab, nr = (None, 0) if ranges is None else (ranges.table, len(ranges))
    _check(load().mrmt3_grad_norm(_p(g), g.numel(), _p(tab), nr, float(grad_scale), float(max_norm),
                                  int(bool(skip_nonfinite)), _p(ws), ws.numel(), _p(stat), _p(skipped), _stream()),
           "grad_norm")


def counter_add(ctr, delta=1):
    """ctr[0] += delta on the device (int32 [1]), stream-ordered: graph-capture safe."""
    _dev(ctr)
    assert ctr.dtype == torch.int32 and ctr.numel() >= 1
    _check(load().mrmt3_counter_add(_p(ctr), int(delta), _stream()), "counter_add")


def transpose(src, out):
    _dev(src, out)
    rows, cols = src.shape
    _check(load().mrmt3_transpose(_p(src), _dt(src), _p(out), _dt(out), rows, cols, _stream()), "transpose")
    return out


def cast(src, out):
    _dev(src, out)
    _check(load().mrmt3_cast(_p(src), _dt(src), _p(out), _dt(out), src.numel(), _stream()), "cast")
    return out


def transpose_batched(src_flat, dst_flat, desc_table, tile_start, n_mats, total_tiles):
    _dev(src_flat, dst_flat, desc_table, tile_start)
    _check(load().mrmt3_transpose_batched(_p(src_flat), _p(dst_flat), _p(desc_table), _p(tile_start), n_mats,
                                          total_tiles, _stream()), "transpose_batched")


COMM_ID_BYTES = 128


class Comm:
    """An RCCL communicator behind the C ABI (`mrmt3_comm_*`, `mrmt3_allreduce`): the gradient exchange of the data-parallel
    step without torch.distributed in the data path (mrmt3/ddp.py, MRMT3_DDP_NATIVE=1).  `uid` = the 128 bytes rank 0 got from
    `Comm.unique_id()`, handed to the other ranks by whatever channel the host has (ddp.py: one broadcast_object_list).
    Creation blocks until every rank has created its end."""

    def __init__(self, uid: bytes, rank: int, world: int):
        assert len(uid) == COMM_ID_BYTES
        self.rank, self.world = rank, world
        self._h = vp()
        buf = C.create_string_buffer(uid, COMM_ID_BYTES)
        _check(load().mrmt3_comm_create(buf, rank, world, C.byref(self._h)), "comm_create")
        # a communicator nobody closed is still destroyed (ncclCommDestroy) when the object goes away or the interpreter
        # exits — before torch's own process group is torn down at exit
        import weakref
        self._fin = weakref.finalize(self, Comm._destroy, self._h)

    @staticmethod
    def _destroy(h):
        if h:
            load().mrmt3_comm_destroy(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(COMM_ID_BYTES)
        _check(load().mrmt3_comm_unique_id(buf), "comm_unique_id")
        return buf.raw

    def allreduce(self, t: torch.Tensor, average: bool = False, stream=None):
        """In place, asynchronous on `stream` (default: the current stream): t = sum (or mean) of t over the ranks."""
        _dev(t)
        assert t.is_contiguous()
        s = C.c_void_p((stream or torch.cuda.current_stream(t.device)).cuda_stream)
        _check(load().mrmt3_allreduce(self._h, _p(t), t.numel(), _dt(t), int(average), s), "allreduce")
        return t

    def close(self):
        if self._h:
            h, self._h = self._h, vp()
            self._fin.detach()
            _check(load().mrmt3_comm_destroy(h), "comm_destroy")


def flag_signal(flag: torch.Tensor, stream=None):
    """flag[0] += 1 behind everything enqueued so far on `stream` (default: the current one) — mrmt3_flag_signal."""
    _dev(flag)
    assert flag.dtype == torch.int32 and flag.numel() >= 1
    s = C.c_void_p((stream or torch.cuda.current_stream(flag.device)).cuda_stream)
    _check(load().mrmt3_flag_signal(_p(flag), s), "flag_signal")


def flag_wait(flag: torch.Tensor, seen: torch.Tensor, err: torch.Tensor, timeout_ms: int = 5000, stream=None):
    """`stream` waits until flag[0] >= seen[0] + 1, then seen[0] += 1; err[0] = 1 after `timeout_ms` without the signal."""
    _dev(flag, seen, err)
    assert flag.dtype == seen.dtype == err.dtype == torch.int32
    s = C.c_void_p((stream or torch.cuda.current_stream(flag.device)).cuda_stream)
    _check(load().mrmt3_flag_wait(_p(flag), _p(seen), _p(err), int(timeout_ms), s), "flag_wait")


# ---- capture hygiene (include/mrmt3_hip.h: "capture hygiene") ------------------------------------------------------------
_CAPTURE_STATUS = {0: "none", 1: "active", 2: "invalidated"}


def stream_capture_status(stream) -> str:
    """'none' / 'active' / 'invalidated' for a torch stream (or a raw handle)."""
    h = stream if isinstance(stream, int) else stream.cuda_stream
    r = load().mrmt3_stream_capture_status(C.c_void_p(h))
    return _CAPTURE_STATUS.get(r, "error(%d)" % r)


def stream_abandon_capture(stream) -> str:
    """End a capture that `stream` is still in (destroying its graph); returns the status before the call."""
    h = stream if isinstance(stream, int) else stream.cuda_stream
    r = load().mrmt3_stream_abandon_capture(C.c_void_p(h))
    return _CAPTURE_STATUS.get(r, "error(%d)" % r)


def runtime_error_pop() -> str:
    """Name of the calling thread's pending HIP runtime error ('' = none); the slot is empty afterwards."""
    buf = C.create_string_buffer(96)
    load().mrmt3_runtime_error_pop(buf, 96)
    return buf.value.decode()


def abort_trace_install(path: str = "") -> None:
    """Opt-in: native frames of the faulting thread on SIGABRT / SIGSEGV (to `path`, default stderr)."""
    _check(load().mrmt3_abort_trace_install(path.encode() if path else None), "abort_trace_install")


class OwnedStream:
    """A HIP stream of our own (mrmt3_stream_create), wrapped for torch as an ExternalStream: NOT from torch's pool of 32 streams
    per priority, which hands a stream that a failed capture left invalidated back out a few dozen `Stream()` calls later.
    `.stream` is the torch handle; close() destroys the HIP stream (call it only when nothing on it is pending)."""

    def __init__(self, device=None, priority: int = 0):
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        h = vp()
        with torch.cuda.device(dev):
            _check(load().mrmt3_stream_create(C.byref(h), int(priority)), "stream_create")
        self.handle, self.device = h.value, dev
        self.stream = torch.cuda.ExternalStream(self.handle, device=dev)

    def close(self):
        h, self.handle = self.handle, None
        if h and _lib is not None:
            self.stream = None
            _lib.mrmt3_stream_destroy(vp(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
