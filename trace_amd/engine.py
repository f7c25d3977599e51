"""Python face of the HIP engine (libtrace_hip.so).  PyTorch is plumbing here: device allocations for the
tensors the caller hands in/out, and the current HIP stream.  All arithmetic happens in the C-ABI library."""
from __future__ import annotations

import contextlib
import ctypes as C
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .config import TraceConfig
from .model.encoders import TimeTower, ScoreTower
from .prefix import APPEND_GROUP_MAX, SHARE_PREFIX_MIN_BATCH, group_by_length, shared_prefix_len, split_questions
from .admit import ADMIT_FRACTION
from .decode_loop import DECODE, DECODE_ROWS, QUEUE, Device, RowBook, checked_requests, decode_loop, flat_forced
from .retire import RETIRE_FRACTION
from .sampling import Constraints, LogitsParams, RowParams, SamplingParams, argmax_rows, check_constraints, ends_stopped, sample_rows_host
from . import scoring

__all__ = ["TraceEngine", "SamplingParams", "ops"]

EPI_NONE, EPI_RESIDUAL, EPI_QUICKGELU, EPI_SWIGLU, EPI_PARTIAL = 0, 1, 2, 3, 4


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _i32(seq) -> "C.Array":
    seq = [int(x) for x in seq]
    return (C.c_int32 * len(seq))(*seq)


class TraceEngine:
    # Batches of at least this many videos prefill the prompt rows they have in common before <video> once and share them (encode_prefill; the
    # break-even: prefix.SHARE_PREFIX_MIN_BATCH).  An instance may set its own.
    share_prefix_min_batch = SHARE_PREFIX_MIN_BATCH
    # Decode steps between two looks at the recorded ids under retire_finished=True (decode): a retire happens at such a boundary only.  An instance may
    # set its own.  With the flag off the loop steps 32 at a time whatever this says.
    retire_chunk = 32
    # ... and a retire happens there once at least 1 / retire_fraction of the running rows have finished (retire.retire_plan, where the reason for the
    # value stands).  An instance may set its own.
    retire_fraction = RETIRE_FRACTION
    # ... and generate_queue admits waiting requests there once the room is at least 1 / admit_fraction of the cap (admit.admit_plan)
    admit_fraction = ADMIT_FRACTION
    # The sampling warpers behind top_p that this engine's sampler applies (csrc/sample.h sample_warp; SamplingParams carries them).  The model class
    # asks before it maps generate()'s arguments of these names: an engine that does not list a warper gets NotImplementedError, never a silent drop.
    sampling_warpers = ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")

    def __init__(self, cfg: TraceConfig, device: int = 0, max_batch: int = 1, max_ctx: Optional[int] = None,
                 max_frames: Optional[int] = None, max_new_tokens: int = 1024, vit_batch_frames: Optional[int] = None,
                 llm_fp8=False, dtype: torch.dtype = torch.bfloat16, kv_cache=None, llm_w4=False):
        """llm_w4: True = the four decoder projections of every layer in the 4-bit "w4" format (trace_amd/w4.py, include/trace_hip.h: e2m1 codes with a
        power-of-two scale per 32 weights), quantised as the weights load and kept as the only copy; prefill dequantises a layer at a time, the decode
        GEMVs widen the codes in registers.  Both multiply by the same matrix, so prefill_append / enable_prefix_cache() / the shared prefix keep their
        bit-identity promise.  bf16 only; not with llm_fp8 or kv_cache; at most 64 sequences decode together.
        kv_cache: None = the KV cache in the 16-bit element type; "fp8" = e4m3 bytes with one fp32 scale per position and kv head (trace_amd/kv8.py:
        264 bytes per position and kv head instead of 512).  Under "fp8" a prefill of whole prompts computes the bits of the 16-bit-cache engine, the
        decode steps attend the quantised rows, and prefill_append / enable_prefix_cache() continue from the QUANTISED prefix: their "bit-identical to
        an uncut prefill" promise is the 16-bit cache's — under "fp8" the guarantee is determinism.  Not with llm_fp8.
        dtype: the 16-bit element type everything is stored and multiplied in — torch.bfloat16 (libtrace_hip.so; north_star's configs) or
        torch.float16 (libtrace_hip_f16.so: the reference's own inference dtype, trace/model/builder.py:50,127,147); accumulation is fp32 in both."""
        # llm_fp8: False / None = bf16 weights; "w8a8" (True is accepted as its alias) = W8A8 prefill GEMMs and decode GEMVs; "weight_only" = W8A8
        # prefill GEMMs, weight-only decode GEMVs (bf16 activations).  Anything else is an error — a typo must not silently pick a numerics scheme.
        if llm_fp8 in (False, None):
            self.fp8_scheme = None
        elif llm_fp8 is True or llm_fp8 == "w8a8":
            self.fp8_scheme = "w8a8"
        elif llm_fp8 == "weight_only":
            self.fp8_scheme = "weight_only"
        else:
            raise ValueError(f"llm_fp8 must be False, True / 'w8a8' or 'weight_only', got {llm_fp8!r}")
        if self.fp8_scheme and dtype != torch.bfloat16:
            raise ValueError("the fp8 weight path exists in the bf16 library only")
        if kv_cache not in (None, "fp8"):
            raise ValueError(f"kv_cache must be None or 'fp8', got {kv_cache!r}")
        if kv_cache and self.fp8_scheme:
            raise ValueError("kv_cache='fp8' with llm_fp8: fp8 weights over an fp8 KV cache is not supported")
        if llm_w4 not in (False, True, None):
            raise ValueError(f"llm_w4 must be False or True, got {llm_w4!r}")
        self.llm_w4 = bool(llm_w4)
        if self.llm_w4 and self.fp8_scheme:
            raise ValueError("llm_w4 with llm_fp8: the decoder projections take one quantised format")
        if self.llm_w4 and kv_cache:
            raise ValueError("llm_w4 with kv_cache='fp8' is not supported")
        if self.llm_w4 and dtype != torch.bfloat16:
            raise ValueError("the w4 weight path exists in the bf16 library only")
        if self.llm_w4 and (cfg.hidden_size % 256 or cfg.intermediate_size % 256):
            raise ValueError("the w4 weight path needs hidden / intermediate sizes that are multiples of 256")
        self.kv_cache = kv_cache
        if not torch.cuda.is_available():
            raise _lib.TraceHipError("no HIP device visible: the TRACE hot path only runs on an MI355X (no CPU fallback)")
        self.dtype = dtype
        self.lib = _lib.load(_lib.element_of(dtype))
        self.cfg = cfg
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        max_frames = max_frames or cfg.num_frames
        if max_ctx is None:
            vis = ((max_frames // 2 + 1) * (cfg.vision_grid // 2 + 1) ** 2 if cfg.mm_projector_type == "stc_connector"
                   else max_frames * cfg.tokens_per_frame)
            max_ctx = min(cfg.max_position_embeddings, vis + 1024 + max_new_tokens)
        self.max_batch, self.max_ctx, self.max_frames, self.max_new_tokens = max_batch, max_ctx, max_frames, max_new_tokens
        if vit_batch_frames is None:
            vit_batch_frames = self.full_round_frames(cfg) if max_batch > 1 else max_frames
        self.vit_batch_frames = max(int(vit_batch_frames), max_frames)
        c = _lib.TraceConfigC(
            cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads,
            cfg.num_key_value_heads, cfg.time_vocab_size, cfg.score_vocab_size, cfg.rms_norm_eps, cfg.rope_theta,
            cfg.vision_hidden_size, cfg.vision_intermediate_size, cfg.vision_layers_used, cfg.vision_num_heads,
            cfg.vision_image_size, cfg.vision_patch_size, cfg.vision_layer_norm_eps, cfg.num_slots, cfg.slot_ln_eps,
            cfg.slot_rope_base, max_frames, max_ctx, max_batch, max_new_tokens,
            1 if cfg.mm_projector_type == "stc_connector" else 0, self.vit_batch_frames,
            {None: 0, "w8a8": 1, "weight_only": 2}[self.fp8_scheme])
        self.llm_fp8 = self.fp8_scheme is not None
        h = C.c_void_p()
        if self.llm_w4:
            o = _lib.TraceCtxOptsW4C(C.sizeof(_lib.TraceCtxOptsW4C), 0, 1)
            _lib.check(self.lib.trace_ctx_create_opts(C.byref(c), device, C.cast(C.byref(o), C.POINTER(_lib.TraceCtxOptsC)), C.byref(h)))
        elif kv_cache:
            o = _lib.TraceCtxOptsC(C.sizeof(_lib.TraceCtxOptsC), 1)
            _lib.check(self.lib.trace_ctx_create_opts(C.byref(c), device, C.byref(o), C.byref(h)))
        else:
            _lib.check(self.lib.trace_ctx_create(C.byref(c), device, C.byref(h)))
        self.h = h
        self.time_tower, self.score_tower = TimeTower(), ScoreTower()
        self._B = 0
        self._max_new = 0
        self._stage_ev = None          # stage_timing(): [(kind, event, event)] while on
        self._stage_videos = 0
        # frames the tower has run / rows prefilled / rows scored so far (what prefix reuse saves is read off these) / rows x steps of the decode_steps
        # calls so far (what retiring finished rows saves is read off that one)
        self.stats = {"vit_frames": 0, "prefill_rows": 0, "score_rows": 0, "decode_row_steps": 0}
        self._rows: List[int] = []            # original index (at decode_begin) of every row of the running decode batch
        self._rows_history: List[List[int]] = []      # _rows after decode_begin and after every retire of the running batch
        self.retires = 0                      # retire_rows calls that shrank a batch, so far
        self.admits = 0                       # admit_rows calls that grew a batch, so far
        self._prefix = None            # (key, rows): KV slot 0 holds `rows` prefilled prompt rows described by `key` (set_prefix_entry); see _prefill_call
        self._dbg = None               # debugging hook: callable(tag, index, tensor-or-None) called between the stages (tools/pipeline_stress.py)

    @property
    def decode_batch_max(self) -> int:
        """sequences one decode batch can hold: the KV slots, at most 256 (64 on the fp8 and w4 weight paths)"""
        return min(self.max_batch, 64 if self.llm_fp8 or self.llm_w4 else self.lib.trace_op_sk_rows())

    @staticmethod
    def full_round_frames(cfg: TraceConfig) -> int:
        """Frames per ViT call when several videos are encoded together: the largest count whose token rows fill 384 row
        tiles of 256 (170 frames x 577 tokens = 383.2 tiles), so that every ViT GEMM — 4 / 12 / 16 column tiles — runs in
        whole rounds of the 256 CUs (6 / 18 / 24) while the fc1 input panel (201 MB) still fits the 256 MB Infinity Cache.
        One 128-frame video alone is 289 row tiles: 4.5 / 13.5 / 18.1 rounds, the last round of each launch half empty.
        Measured (tools/vit_chunk_sweep.py, tower ms per video): 128 -> 55.0, 170 -> 53.9, 227 (512 tiles; the fc1 panel
        spills the cache: 931 vs 979 TFLOP/s on that launch) -> 53.6, 64 -> 58.6."""
        return max(1, min(256, (384 * 256) // cfg.vision_tokens))

    def close(self):
        if getattr(self, "h", None):
            self.lib.trace_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- weights -------------------------------------------------------------------------------
    def load_weights(self, items: Iterable[Tuple[str, torch.Tensor]]) -> int:
        """items: (reference state-dict name, tensor).  Tensors are converted to the engine's contiguous 16-bit dtype; host or device."""
        n = 0
        for name, t in items:
            t = t.detach().to(self.dtype).contiguous()
            shape = (C.c_int64 * max(t.dim(), 1))(*(list(t.shape) or [1]))
            rc = _lib.check(self.lib.trace_ctx_load_tensor(self.h, name.encode(), C.c_void_p(t.data_ptr()),
                                                          1 if t.is_cuda else 0, shape, t.dim()))
            n += rc == 0
        _lib.check(self.lib.trace_ctx_finalize(self.h))
        return n

    def device_bytes(self) -> int:
        return int(self.lib.trace_ctx_device_bytes(self.h))

    # ---- stages --------------------------------------------------------------------------------
    def _frames(self, frames: torch.Tensor):
        if frames.dim() != 4:
            raise ValueError("frames must be [T,3,H,W]")
        if frames.dtype not in (self.dtype, torch.float32):
            frames = frames.to(self.dtype)
        frames = frames.to(self.device).contiguous()
        return frames, (1 if frames.dtype == torch.float32 else 0)

    CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
    CLIP_STD = (0.26862954, 0.26130258, 0.27577711)

    def preprocess_frames(self, frames_u8, pad: bool = True, image_mean: Sequence[float] = CLIP_MEAN,
                          image_std: Sequence[float] = CLIP_STD, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """process_video's per-frame image work (mm_utils.py:456-462) on the device: uint8 RGB [T,H,W,3] (tensor or numpy,
        host or device) -> [T,3,S,S] `dtype` (bf16 for the engine, fp32 = the reference's FloatTensor bit for bit)."""
        x = torch.as_tensor(frames_u8)
        if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[-1] != 3:
            raise ValueError(f"expected uint8 [T,H,W,3] RGB frames, got {x.dtype} {tuple(x.shape)}")
        dtype = dtype or self.dtype
        if dtype not in (self.dtype, torch.float32):
            raise ValueError(f"dtype must be the engine's {self.dtype} or float32")
        x = x.to(self.device).contiguous()
        T, H, W, _ = x.shape
        S = self.cfg.vision_image_size
        out = torch.empty((T, 3, S, S), dtype=dtype, device=self.device)
        mean, std = (C.c_float * 3)(*image_mean), (C.c_float * 3)(*image_std)
        _lib.check(self.lib.trace_preprocess_frames(self.h, _ptr(x), T, H, W, int(bool(pad)), mean, std, _ptr(out),
                                                    1 if dtype == torch.float32 else 0, _stream()))
        return out

    def vit_forward(self, frames: torch.Tensor, want_output: bool = True) -> Optional[torch.Tensor]:
        frames, dt = self._frames(frames)
        T = frames.shape[0]
        self.stats["vit_frames"] += T
        if not want_output:
            _lib.check(self.lib.trace_vit_forward(self.h, _ptr(frames), dt, T, None, _stream()))
            return None
        out = torch.empty((T, self.cfg.vision_patches, self.cfg.vision_hidden_size), dtype=self.dtype, device=self.device)
        _lib.check(self.lib.trace_vit_forward(self.h, _ptr(frames), dt, T, _ptr(out), _stream()))
        return out

    def slot_pool(self, feats: Optional[torch.Tensor], T: int) -> torch.Tensor:
        out = torch.empty((T, self.cfg.num_slots, self.cfg.hidden_size), dtype=self.dtype, device=self.device)
        if feats is not None:
            feats = feats.to(self.device, self.dtype).contiguous()
        _lib.check(self.lib.trace_slot_pool(self.h, _ptr(feats), T, _ptr(out), _stream()))
        return out

    def stc_connector(self, feats: Optional[torch.Tensor], T: int) -> torch.Tensor:
        """Legacy STC connector (projector_type 'stc_connector'); result also becomes the video rows for splice()."""
        self._drop_prefix()
        g = self.cfg.vision_grid // 2 + 1
        rows = (T // 2 + 1) * g * g
        out = torch.empty((rows, self.cfg.hidden_size), dtype=self.dtype, device=self.device)
        if feats is not None:
            feats = feats.to(self.device, self.dtype).contiguous()
        n = C.c_int(0)
        _lib.check(self.lib.trace_stc_connector(self.h, _ptr(feats), T, _ptr(out), C.byref(n), _stream()))
        assert n.value == rows
        return out

    def time_ids(self, timestamps: Sequence[Sequence[float]]) -> List[int]:
        """encode_time + [:-1] (trace_arch.py:243,271-288): 6 ids per frame; all frames must agree in length."""
        toks = [self.time_tower.encode_ids(t) for t in timestamps]
        assert all(len(x) == len(toks[0]) for x in toks), f"{timestamps} {[len(x) for x in toks]}"
        if len(toks[0]) - 1 != self.cfg.time_tokens_per_frame:
            raise ValueError("each frame must carry exactly one timestamp (6 time tokens)")
        return [i for x in toks for i in x[:-1]]

    def encode_video(self, frames: torch.Tensor, timestamps, want_output: bool = False):
        self._drop_prefix()
        frames, dt = self._frames(frames)
        T = frames.shape[0]
        self.stats["vit_frames"] += T
        ids = _i32(self.time_ids(timestamps))
        out = None
        if want_output:
            out = torch.empty((T * self.cfg.tokens_per_frame, self.cfg.hidden_size), dtype=self.dtype, device=self.device)
        _lib.check(self.lib.trace_encode_video(self.h, _ptr(frames), dt, T, ids, _ptr(out), _stream()))
        return out

    def encode_features(self, feats: torch.Tensor, timestamps, want_output: bool = False):
        """encode_video from ViT features computed earlier (vit_forward on a frame batch that may span several videos)"""
        self._drop_prefix()
        T = feats.shape[0]
        assert feats.dtype == self.dtype and feats.is_cuda and feats.is_contiguous()
        ids = _i32(self.time_ids(timestamps))
        out = None
        if want_output:
            out = torch.empty((T * self.cfg.tokens_per_frame, self.cfg.hidden_size), dtype=self.dtype, device=self.device)
        _lib.check(self.lib.trace_encode_features(self.h, _ptr(feats), T, ids, _ptr(out), _stream()))
        return out

    def vit_forward_many(self, videos: Sequence[torch.Tensor]) -> List[torch.Tensor]:
        """ViT features of several videos, the frames pushed through the tower `vit_batch_frames` at a time regardless of
        video boundaries (per-frame arithmetic: identical to per-video calls).  Returns one [T_v, patches, v_hidden] view
        per video."""
        vids = [self._frames(v) for v in videos]
        dts = {dt for _, dt in vids}
        if len(dts) != 1:
            raise ValueError("all videos of a batch must share one frame dtype")
        dt = dts.pop()
        counts = [v.shape[0] for v, _ in vids]
        total = sum(counts)
        feats = torch.empty((total, self.cfg.vision_patches, self.cfg.vision_hidden_size), dtype=self.dtype, device=self.device)
        F = self.vit_batch_frames
        pos, chunk, chunk_n = 0, [], 0          # gather frames into chunks of F (a copy only when a chunk spans videos)
        def flush():
            nonlocal chunk, chunk_n, pos
            if not chunk_n:
                return
            x = chunk[0] if len(chunk) == 1 else torch.cat(chunk, dim=0)
            self.stats["vit_frames"] += chunk_n
            _lib.check(self.lib.trace_vit_forward(self.h, _ptr(x.contiguous()), dt, chunk_n, _ptr(feats[pos:pos + chunk_n]), _stream()))
            pos += chunk_n
            chunk, chunk_n = [], 0
        for v, _ in vids:
            o = 0
            while o < v.shape[0]:
                n = min(F - chunk_n, v.shape[0] - o)
                chunk.append(v[o:o + n])
                chunk_n += n
                o += n
                if chunk_n == F:
                    flush()
        flush()
        out, o = [], 0
        for n in counts:
            out.append(feats[o:o + n])
            o += n
        return out

    def splice(self, input_ids: Sequence[int], time_rows: Sequence[int] = (), score_rows: Sequence[int] = (),
               want_output: bool = False):
        ids = _i32(input_ids)
        tr, sr = _i32(time_rows), _i32(score_rows)
        L = C.c_int(0)
        # length is known up-front: n_ids - 1 + video rows; allocate generously when a copy is requested
        out = None
        if want_output:
            out = torch.empty((self.max_ctx, self.cfg.hidden_size), dtype=self.dtype, device=self.device)
        _lib.check(self.lib.trace_splice_embeds(self.h, ids, len(ids), tr, len(tr), sr, len(sr), C.byref(L), _ptr(out), _stream()))
        return (L.value, out[: L.value]) if want_output else L.value

    # The model's prefix cache (TraceMistralForCausalLM.enable_prefix_cache) keeps its one entry in KV slot 0.  Whether the slot still holds those rows is
    # decided here: every call that rewrites slot 0 from row 0 or below the entry's length, or encodes a video (the entry's owner then no longer knows
    # which video the engine last saw), drops it.  Decoding never does: it writes rows at and above the slot's length.
    def _prefill_call(self, call: str, slot0: int, past: int, tensors, L: int, want_hidden: bool = False, src=None, score=()):
        """One prefill pass through the C symbol trace_llm_<call>: the pointer array of `tensors` (contiguous device [L, hidden] rows of this engine's
        dtype, one per slot; None: the engine's own embedding buffer, one slot), the prefix-entry rule, stats["prefill_rows"].  Returns the [L, hidden]
        final-norm rows if want_hidden.  src: prefill_shared's source slot; score: score_append's (heads, ids, out)."""
        n = len(tensors) if tensors else 1
        ptrs = (C.c_void_p * n)(*[e.data_ptr() for e in tensors]) if tensors else None
        hid = torch.empty((L, self.cfg.hidden_size), dtype=self.dtype, device=self.device) if want_hidden else None
        if call in ("prefill_append", "score_append"):                 # rows below `past` stay: the entry survives unless they reach into it
            drop = slot0 == 0 and self._prefix is not None and past < self._prefix[1]
        else:                                                          # a whole prompt, or the shared rows copied in, from row 0
            drop = slot0 == 0
        if drop:
            self._drop_prefix()
        args = {"prefill": lambda: (slot0, ptrs and ptrs[0], L, _ptr(hid)),
                "prefill_pair": lambda: (slot0, ptrs[0], ptrs[1], L),
                "prefill_multi": lambda: (slot0, ptrs, n, L),
                "prefill_append": lambda: (slot0, n, past, ptrs, L, _ptr(hid)),
                "prefill_shared": lambda: (src, slot0, n, past, ptrs, L),
                "score_append": lambda: (slot0, n, past, ptrs, L, *score)}[call]()
        _lib.check(getattr(self.lib, "trace_llm_" + call)(self.h, *args, _stream()))
        self.stats["prefill_rows"] += n * L
        return hid

    def prefill(self, slot: int, L: int, embeds: Optional[torch.Tensor] = None, want_hidden: bool = False):
        keep = None if embeds is None else [embeds.to(self.device, self.dtype).contiguous()]
        return self._prefill_call("prefill", slot, 0, keep, L, want_hidden)

    # ---- prompt-prefix reuse: continue a slot that holds rows, copy rows between slots, embed rows without a video ----
    def embed_rows(self, ids: Sequence[int], time_rows: Sequence[int] = (), score_rows: Sequence[int] = (), want_output: bool = False):
        """splice() for rows that hold no <video> (trace_embed_rows): the embeddings stay in the engine's buffer for prefill_append(embeds=None);
        want_output returns a copy [len(ids), hidden]."""
        arr, tr, sr = _i32(ids), _i32(time_rows), _i32(score_rows)
        out = torch.empty((len(arr), self.cfg.hidden_size), dtype=self.dtype, device=self.device) if want_output else None
        _lib.check(self.lib.trace_embed_rows(self.h, arr, len(arr), tr, len(tr), sr, len(sr), _ptr(out), _stream()))
        return out

    def prefill_append(self, slot0: int, past: int, embeds=None, L: Optional[int] = None, want_hidden: bool = False):
        """L new rows at positions past .. past + L - 1 of slots slot0 .. slot0 + n - 1, each of which holds at least `past` rows
        (trace_llm_prefill_append).  embeds: one [L, hidden] tensor, a list of up to 8 of equal shape (one per slot), or None = the rows of the
        last embed_rows() (then L is required).  want_hidden (one slot): the [L, hidden] final-norm rows."""
        if embeds is None:
            if L is None:
                raise ValueError("prefill_append(embeds=None) needs L, the row count of the last embed_rows()")
            keep, n = None, 1
        else:
            keep = [e.to(self.device, self.dtype).contiguous() for e in ([embeds] if isinstance(embeds, torch.Tensor) else list(embeds))]
            n = len(keep)
            if not 1 <= n <= APPEND_GROUP_MAX or any(e.dim() != 2 or e.shape != keep[0].shape or e.shape[1] != self.cfg.hidden_size for e in keep):
                raise ValueError(f"embeds: 1 to {APPEND_GROUP_MAX} tensors of one shape [L, hidden]")
            L = keep[0].shape[0]
        if want_hidden and n != 1:
            raise ValueError("want_hidden with one slot only")
        return self._prefill_call("prefill_append", int(slot0), int(past), keep, int(L), want_hidden)

    def kv_copy(self, src: int, dsts: Sequence[int], rows: int):
        """KV rows [0, rows) of slot `src` to every slot of `dsts` (trace_kv_copy); their length becomes `rows`."""
        dsts = [int(d) for d in dsts]
        if 0 in dsts:
            self._drop_prefix()
        _lib.check(self.lib.trace_kv_copy(self.h, int(src), _i32(dsts), len(dsts), int(rows), _stream()))

    def prefill_shared(self, src: int, slot0: int, past: int, embeds: Sequence[torch.Tensor]):
        """A run of a batch that shares its first `past` prompt rows, held by slot `src` (trace_llm_prefill_shared): the rows are copied to slots
        slot0 .. slot0 + n - 1 (those that are not `src`) and every slot continues with its own rows embeds[i] [L, hidden] (equal shapes)."""
        keep = [e.contiguous() for e in embeds]
        n = len(keep)
        assert 1 <= n <= APPEND_GROUP_MAX and all(e.shape == keep[0].shape and e.dtype == self.dtype and e.is_cuda for e in keep)
        self._prefill_call("prefill_shared", int(slot0), int(past), keep, keep[0].shape[0], src=int(src))

    def set_prefix_entry(self, key, rows: int):
        self._prefix = (key, int(rows))

    def prefix_entry(self):
        return self._prefix

    def _drop_prefix(self):
        self._prefix = None

    def head_logits(self, hidden: torch.Tensor, head: int) -> torch.Tensor:
        """masked fp32 logits [R, total_vocab] of final-norm hidden rows under one head (forward()'s logits at every position)"""
        assert hidden.dtype == self.dtype and hidden.is_cuda and hidden.is_contiguous()
        out = torch.empty((hidden.shape[0], self.cfg.total_vocab), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trace_llm_head_logits(self.h, _ptr(hidden), hidden.shape[0], int(head), _ptr(out), _stream()))
        return out

    # ---- scoring given tokens (trace_llm_score_rows / trace_llm_score_append; include/trace_hip.h states the semantics) ----
    def score_rows(self, hidden: torch.Tensor, heads: Sequence[int], ids: Sequence[int]) -> np.ndarray:
        """float32 [R]: the log-probability of ids[r] under head heads[r] from final-norm hidden row r (the rows prefill(want_hidden=True) returns);
        id -1 gives 0.0, an id outside the head -inf.  No [R, vocabulary] logits are ever stored."""
        assert hidden.dtype == self.dtype and hidden.is_cuda and hidden.is_contiguous() and hidden.dim() == 2 and hidden.shape[1] == self.cfg.hidden_size
        R = hidden.shape[0]
        if len(heads) != R or len(ids) != R:
            raise ValueError("one head and one id per hidden row")
        hd = torch.tensor([int(h) for h in heads], dtype=torch.int32, device=self.device)
        ii = torch.tensor([int(t) for t in ids], dtype=torch.int32, device=self.device)
        out = torch.empty(R, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trace_llm_score_rows(self.h, _ptr(hidden), R, _ptr(hd), _ptr(ii), _ptr(out), _stream()))
        self.stats["score_rows"] += R
        return out.cpu().numpy()

    def score_continuations(self, slot0: int, past_rows: int, last_prompt_embed_row: torch.Tensor, continuations: Sequence[Sequence[int]], head=1,
                            pad_id: int = 0):
        """Log-probabilities of given continuations of ONE prompt of past_rows rows.  last_prompt_embed_row: the embedding of the prompt's last row
        [hidden] — or of its last k rows [k, hidden] — while slot slot0 holds the past_rows - k rows before them (it may hold more: they are rewritten).
        Continuation b's appended rows are [those k rows, embed(c[0]), ..., embed(c[n_b - 2])] at positions past_rows - k ..., so the row at position
        past_rows - 1 + i predicts c[i] under head_chain(c, head)[i] (head: one int, or one per continuation).  Continuations of unequal length are
        padded to the group's longest with pad_id (any text id) and target -1: the padding follows the real rows, so causality keeps it from
        touching them.  Groups of up to 8 consecutive slots slot0 ..., each group within the prefill workspace, the prefix fanned out with
        kv_copy; one trace_llm_score_append per group.  Returns ([float32 array per continuation], [head list per continuation], float64 sums).
        Afterwards the slots hold rows that belong to the continuations: only rows below past_rows - k of slot0 are still the prompt's."""
        cfg = self.cfg
        rows = last_prompt_embed_row.to(self.device, self.dtype)
        rows = rows.unsqueeze(0) if rows.dim() == 1 else rows
        if rows.dim() != 2 or rows.shape[1] != cfg.hidden_size or rows.shape[0] < 1:
            raise ValueError("last_prompt_embed_row: [hidden] or [k, hidden]")
        k = rows.shape[0]
        past = int(past_rows) - k
        if past < 0:
            raise ValueError("past_rows counts the whole prompt: it cannot be smaller than the rows handed in")
        nc = len(continuations)
        if nc < 1:
            raise ValueError("no continuation to score")
        heads0 = [int(head)] * nc if isinstance(head, (int, np.integer)) else [int(h) for h in head]
        if len(heads0) != nc:
            raise ValueError("one starting head, or one per continuation")
        conts = [scoring.check_continuation(cfg, c, h) for c, h in zip(continuations, heads0)]
        if not 0 <= int(pad_id) < cfg.vocab_size:
            raise ValueError("pad_id must be a text id")
        longest = max(len(c) for c in conts)
        if past + k - 1 + longest > self.max_ctx:
            raise ValueError(f"prompt ({past_rows} rows) + continuation ({longest} tokens) exceeds max_ctx {self.max_ctx}")
        gmax = min(APPEND_GROUP_MAX, self.max_batch - int(slot0))
        if gmax < 1:
            raise ValueError("slot0 outside the engine's KV slots")
        chains = [scoring.head_chain(cfg, c, h) for c, h in zip(conts, heads0)]
        out = [None] * nc
        for run in scoring.groups_of([k - 1 + len(c) for c in conts], self.prefill_rows, gmax):
            L = k - 1 + max(len(conts[b]) for b in run)
            embeds, hd, tg = [], [], []
            for b in run:
                fed = scoring.fed_ids(conts[b], L - (k - 1), pad_id)
                e = rows
                if fed:
                    e = torch.cat([rows, self.embed_rows(*scoring.embed_placeholders(cfg, fed), want_output=True)], 0)
                embeds.append(e.contiguous())
                t, h = scoring.targets(conts[b], chains[b], L - (k - 1))
                tg += [scoring.IGNORE] * (k - 1) + t
                hd += [0] * (k - 1) + h
            n = len(run)
            if n > 1 and past > 0:
                self.kv_copy(slot0, list(range(slot0 + 1, slot0 + n)), past)
            res = (C.c_float * (n * L))()
            self._prefill_call("score_append", int(slot0), past, embeds, L, score=(_i32(hd), _i32(tg), res))
            self.stats["score_rows"] += n * L
            arr = np.frombuffer(res, dtype=np.float32).reshape(n, L)
            for j, b in enumerate(run):
                out[b] = arr[j, k - 1:k - 1 + len(conts[b])].copy()
        sums = np.array([np.sum(o, dtype=np.float64) for o in out], np.float64)
        return out, chains, sums

    def prefill_pair(self, slot0: int, embeds0: torch.Tensor, embeds1: torch.Tensor):
        """two spliced prompts of equal length -> KV slots slot0, slot0 + 1 in one pass (trace_llm_prefill_pair)"""
        assert embeds0.shape == embeds1.shape and embeds0.dtype == self.dtype and embeds0.is_cuda
        self._prefill_call("prefill_pair", slot0, 0, [embeds0.contiguous(), embeds1.contiguous()], embeds0.shape[0])

    PREFILL_GROUP = 4          # equal-length prompts of max_ctx rows one prefill pass takes (trace_llm_prefill_multi); shorter prompts: prefill_group(L)
    PREFILL_GROUP_MAX = 8

    @property
    def prefill_rows(self) -> int:
        """rows the prefill workspaces hold (engine.hip pf_rows): n prompts of L rows fit one pass while n * L <= this"""
        return max(self.PREFILL_GROUP * self.max_ctx, min(8192, self.PREFILL_GROUP_MAX * self.max_ctx))

    def prefill_group(self, L: int) -> int:
        """How many equal-length prompts of L rows to put through one prefill pass: the n <= 8 that fits the workspaces and minimises the projections' cost per
        prompt in whole rounds of the 256 CUs — a 256 x 256 tile occupies a CU for one tile time whether its round is full or not, so cost(n) = sum over the four
        projections of ceil(row panels x column tiles / #CUs) x K.  C2 (L = 1967): 4 (31 row panels; 8 would not fit).  C4 (L = 1086): 7 (30 panels: the o / down
        grid in 1.9 rounds; four prompts' 17 panels take 2 rounds for 1.06 of work: -22 % of the projections' time per prompt)."""
        c = self.cfg
        H, I = c.hidden_size, c.intermediate_size
        qkv = (c.num_attention_heads + 2 * c.num_key_value_heads) * (H // c.num_attention_heads)
        shapes = ((qkv, H), (H, H), (2 * I, H), (H, I))          # (N, K) of qkv, o, gate|up, down
        ncu = 256
        best, best_cost = 1, None
        for n in range(1, self.PREFILL_GROUP_MAX + 1):
            if n * L > self.prefill_rows:
                break
            panels = -(-n * L // 256)
            cost = sum(-(-panels * -(-N // 256) // ncu) * K for N, K in shapes) / n
            if best_cost is None or cost < best_cost * 0.995:      # (ties go to the smaller group: less latency to the first prefilled slot)
                best, best_cost = n, cost
        return best

    def prefill_multi(self, slot0: int, embeds: Sequence[torch.Tensor]):
        """up to 8 spliced prompts of equal length, n x L within prefill_rows -> KV slots slot0 .. slot0 + n - 1 in one pass (trace_llm_prefill_multi)"""
        n = len(embeds)
        assert 1 <= n <= self.PREFILL_GROUP_MAX and n * embeds[0].shape[0] <= self.prefill_rows and all(e.shape == embeds[0].shape and e.dtype == self.dtype and e.is_cuda for e in embeds)
        self._prefill_call("prefill_multi", slot0, 0, [e.contiguous() for e in embeds], embeds[0].shape[0])

    # ---- decode --------------------------------------------------------------------------------
    def decode_begin(self, slots: Sequence[int], heads: Sequence[int], max_new: int, eos: int = -1,
                     forced: Optional[Sequence[Sequence[int]]] = None, want_logits: bool = False, shared_prefix=None,
                     row_params: Optional[Sequence[RowParams]] = None):
        """shared_prefix: (slot, rows) as encode_prefill returns it — every slot of the batch holds the same first `rows` rows, `slot` among them:
        the decode attention reads whole 32-position blocks of them from that slot alone (trace_decode_set_shared_prefix).
        row_params: one RowParams per row (trace_decode_set_row_params) — every row samples (or not) under its own params and seed, runs its own
        logits processors and stops recording at its own max_new_tokens; set_sampling / set_logits_params are ignored by such a batch, and rows join
        it through admit_rows_ex only.  None: the batch-wide settings, as ever."""
        B = len(slots)
        rp = None
        if row_params is not None:
            if len(row_params) != B:
                raise ValueError("one RowParams per row of the batch")
            rp = row_params_c(list(row_params), max_new)
        if shared_prefix is not None:
            _lib.check(self.lib.trace_decode_set_shared_prefix(self.h, int(shared_prefix[0]), int(shared_prefix[1]) & ~31))
        self._B, self._max_new = B, max_new
        self._rows = list(range(B))
        self._rows_history = [list(self._rows)]
        f = None if forced is None else _i32(flat_forced(forced, max_new))
        lg = torch.empty((B, self.cfg.total_vocab), dtype=torch.float32, device=self.device) if want_logits else None
        if rp is not None:
            _lib.check(self.lib.trace_decode_set_row_params(self.h, rp, B))
        try:
            _lib.check(self.lib.trace_decode_begin(self.h, _i32(slots), B, _i32(heads), max_new, eos, f, _ptr(lg), _stream()))
        finally:
            if rp is not None:               # (a begin that failed before it looked at the request must not leave it to the next one)
                self.lib.trace_decode_set_row_params(self.h, None, 0)
        return lg

    def decode_steps(self, n: int, use_graph: bool = True, want_logits: bool = False):
        lg = None
        if want_logits:
            lg = torch.empty((self._B, self.cfg.total_vocab), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.trace_decode_steps(self.h, n, 1 if use_graph else 0, _ptr(lg), _stream()))
        self.stats["decode_row_steps"] += self._B * n
        return lg

    def retire_rows(self, keep: Sequence[int]):
        """Shrink the running decode batch to the rows at positions `keep` (strictly increasing, within the current batch; trace_decode_retire):
        everything a step holds per row moves with the row, and a sampled row goes on drawing with the Philox row index it began with.  Read the
        results of the rows that leave first (decode_read, decode_read_logprobs): afterwards those return len(keep) rows.  self._rows keeps the
        original index of every live row.  All rows in order = nothing happens.  Not in host-select mode."""
        keep = [int(k) for k in keep]
        _lib.check(self.lib.trace_decode_retire(self.h, _i32(keep), len(keep), _stream()))
        shrunk = len(keep) != self._B
        self._rows = [self._rows[k] for k in keep]
        self._B = len(keep)
        if shrunk:
            self.retires += 1
            self._rows_history.append(list(self._rows))

    def admit_rows(self, slots: Sequence[int], heads: Sequence[int], row_ids: Optional[Sequence[int]] = None,
                   forced: Optional[Sequence[Sequence[int]]] = None):
        """Append prefilled KV slots behind the rows of the running decode batch (trace_decode_admit): the new rows get what decode_begin gives a
        batch, their token 0 is selected on them alone, and from there each counts steps of its own: ids, length, forced ids, log-probabilities,
        min_new_tokens, begin_suppress_tokens, the stop match and the sampler's counter are those of a row begun at its step 0.  row_ids: the Philox
        row index of each new row (default: the position it lands at), so a sampled row can draw what that row of a batch begun together draws.
        self._rows names the new rows by the next unused original indices.  Retire first, then admit.  Not in host-select mode, not under a shared
        prefix, not with forced ids while processors or constraints are armed.  Into a batch begun with row_params: admit_rows_ex."""
        self._admit(slots, heads, row_ids, forced, None)

    def admit_rows_ex(self, slots: Sequence[int], heads: Sequence[int], row_params: Sequence[RowParams], row_ids: Optional[Sequence[int]] = None,
                      forced: Optional[Sequence[Sequence[int]]] = None):
        """admit_rows into a batch begun with row_params (and only into such a batch: trace_decode_admit_ex): one RowParams per admitted row, written
        beside the batch's before the rows' token 0 is selected.  Forced ids are refused only for a row whose processors are armed, or under constraints."""
        if row_params is None:
            raise ValueError("admit_rows_ex takes one RowParams per admitted slot (admit_rows admits into a batch begun without them)")
        self._admit(slots, heads, row_ids, forced, row_params)

    def _admit(self, slots, heads, row_ids, forced, row_params):
        slots, heads = [int(s) for s in slots], [int(h) for h in heads]
        n, mn = len(slots), self._max_new
        if len(heads) != n or (row_ids is not None and len(row_ids) != n) or (forced is not None and len(forced) != n) or \
                (row_params is not None and len(row_params) != n):
            raise ValueError("one head, row index, forced row and RowParams per admitted slot")
        rid = [int(r) for r in row_ids] if row_ids is not None else list(range(self._B, self._B + n))
        f = None if forced is None else _i32(flat_forced(forced, mn))
        if row_params is None:
            _lib.check(self.lib.trace_decode_admit(self.h, _i32(slots), n, _i32(heads), _i32(rid), f, _stream()))
        else:
            _lib.check(self.lib.trace_decode_admit_ex(self.h, _i32(slots), n, _i32(heads), _i32(rid), f, row_params_c(list(row_params), mn), _stream()))
        nxt = 1 + max([max(h) for h in self._rows_history if h] + [-1])
        self._rows = self._rows + list(range(nxt, nxt + n))
        self._B += n
        self.admits += 1
        self._rows_history.append(list(self._rows))

    def decode_read(self):
        B, mn = self._B, self._max_new
        ids = (C.c_int32 * (B * mn))()
        ln = (C.c_int32 * B)()
        hd = (C.c_int32 * B)()
        _lib.check(self.lib.trace_decode_read(self.h, ids, ln, hd, _stream()))
        out = [[ids[b * mn + i] for i in range(ln[b])] for b in range(B)]
        return out, list(hd)

    def set_logprobs(self, on: bool):
        """Per-token log-probabilities for the decode batches begun from now on (trace_decode_set_logprobs): the device computes, inside every
        decode step, log softmax of the RAW masked logits of the row's active head at the emitted id (sampling.token_logprob_ref, bit for bit)."""
        _lib.check(self.lib.trace_decode_set_logprobs(self.h, 1 if on else 0))

    def decode_read_logprobs(self, lengths: Optional[Sequence[int]] = None):
        """float32 [B, max_new] of the current batch (0.0 past a row's length); with `lengths`: one array per row, cut to that row's length"""
        B, mn = self._B, self._max_new
        out = np.zeros((B, mn), np.float32)
        _lib.check(self.lib.trace_decode_read_logprobs(self.h, out.ctypes.data_as(C.c_void_p), _stream()))
        if lengths is None:
            return out
        return [out[b, : int(n)].copy() for b, n in enumerate(lengths)]

    def token_logprob(self, logits: torch.Tensor, heads: Sequence[int], ids: Sequence[int]) -> np.ndarray:
        """float32 [B]: the log-probability of ids[b] under row b of masked logits [B, NV] fp32 (device) and head heads[b] (trace_op_token_logprob:
        the device code of the decode step) - the host-driven paths call it on the logits they bring back."""
        cfg = self.cfg
        out = ops.token_logprob(logits, heads, ids, cfg.vocab_size, cfg.time_vocab_size, cfg.score_vocab_size, element=_lib.element_of(self.dtype))
        return out.cpu().numpy()

    def host_mode(self, on: bool):
        """Host-driven token selection (sampling / stopping criteria): logits come back every step, ids go in via feed()."""
        _lib.check(self.lib.trace_decode_host_mode(self.h, 1 if on else 0))

    def feed(self, tokens: Sequence[int]):
        _lib.check(self.lib.trace_decode_feed(self.h, _i32(tokens), len(tokens), _stream()))

    def set_sampling(self, sampling: Optional[SamplingParams]):
        """Device sampling for the decode batches begun from now on (trace_decode_set_sampling_ex); None or temperature <= 0 = greedy.
        Only parameters inside the device sampler's domain (SamplingParams.on_device) are accepted here; decode() routes the others."""
        if sampling is None or sampling.greedy:
            _lib.check(self.lib.trace_decode_set_sampling(self.h, 0.0, 0, 1.0, 0))
        else:
            _lib.check(self.lib.trace_decode_set_sampling_ex(self.h, C.byref(sampling_c(sampling))))

    def set_logits_params(self, logits: Optional[LogitsParams]):
        """Logits processors for the decode batches begun from now on (trace_decode_set_logits_params): repetition penalty, no-repeat n-grams and
        min_new_tokens over the ids a row has generated so far, applied on the device between the head logits and the token selection.  None or
        LogitsParams() disarms them."""
        lp = logits if logits is not None else LogitsParams()
        _lib.check(self.lib.trace_decode_set_logits_params(self.h, float(lp.repetition_penalty), int(lp.no_repeat_ngram_size), int(lp.min_new_tokens)))

    def logits_process(self, logits: torch.Tensor, heads: Sequence[int], hist: Sequence[Sequence[int]], params: LogitsParams, steps: Sequence[int],
                       eos: int = -1) -> torch.Tensor:
        """Masked logits [B, NV] fp32 (device) -> a new tensor of the same shape: row b processed as a decode step processes it at device step
        steps[b] with history hist[b] (trace_op_logits_process: the device code of the decode step; sampling.process_row_ref bit for bit) - the
        host-driven paths call it on the logits they bring back."""
        cfg = self.cfg
        return ops.logits_process(logits, heads, hist, params, steps, eos, cfg.vocab_size, cfg.time_vocab_size, cfg.score_vocab_size,
                                  element=_lib.element_of(self.dtype))

    def set_constraints(self, constraints: Optional[Constraints]):
        """Bad words, suppressed ids and stop sequences for the decode batches begun from now on (trace_decode_set_constraints, csrc/constrain.h):
        the bans join the logits processors' launch, the stop sequences end a row inside the selection as EOS does.  None or Constraints()
        disarms them.  ValueError for an id outside the vocabulary or a list beyond the device's bounds."""
        if constraints is None or constraints.off:
            _lib.check(self.lib.trace_decode_set_constraints(self.h, None))
            return
        k, keep = constraints_c(constraints, self.cfg.total_vocab)
        _lib.check(self.lib.trace_decode_set_constraints(self.h, C.byref(k)))
        del keep

    def logits_process_ex(self, logits: torch.Tensor, heads: Sequence[int], hist: Sequence[Sequence[int]], params: Optional[LogitsParams],
                          steps: Sequence[int], eos: int = -1, constraints: Optional[Constraints] = None) -> torch.Tensor:
        """logits_process with the ban rules of `constraints` behind the processors (trace_op_logits_process_ex: the device code of the decode step;
        sampling.constrain_row_ref of sampling.process_row_ref)."""
        cfg = self.cfg
        return ops.logits_process_ex(logits, heads, hist, params, steps, eos, constraints, cfg.vocab_size, cfg.time_vocab_size, cfg.score_vocab_size,
                                     element=_lib.element_of(self.dtype))

    def sample(self, logits: torch.Tensor, heads: Sequence[int], sampling: SamplingParams, steps: Sequence[int]) -> List[int]:
        """One id per row of masked logits [B, NV] fp32 (device), drawn as a decode step draws them (row b: Philox step steps[b], row index b):
        the device sampler (trace_op_sample) inside its domain, the host statement of the same rules outside it."""
        cfg = self.cfg
        if not sampling.on_device:
            return sample_rows_host(logits, heads, cfg.vocab_size, cfg.time_vocab_size, cfg.score_vocab_size, sampling, steps)
        out = ops.sample(logits, heads, sampling, steps, cfg.vocab_size, cfg.time_vocab_size, cfg.score_vocab_size, element=_lib.element_of(self.dtype))
        return out.tolist()

    def set_profile(self, mode: int):
        """0 off; 1 time decode_steps calls; 2 also bracket one gate|up GEMV launch per decode step with HIP events."""
        _lib.check(self.lib.trace_set_profile(self.h, int(mode)))

    def get_profile(self) -> List[float]:
        buf = (C.c_float * 20)()
        _lib.check(self.lib.trace_get_profile(self.h, buf, 20))
        return list(buf)

    # ---- one-call convenience: what generate() does for one batch of videos ----------------------
    # ---- stage timing inside a run (bench.py): HIP-event pairs around the tower / slot-pool / prefill calls of encode_prefill ----
    def stage_timing(self, on: bool):
        """on: encode_prefill brackets its tower, encode_features and prefill calls with event pairs on its stream (generate(): every batch;
        generate_stream(): only the batch that fills the pipeline, while the encode stage has the GPU to itself); read with stage_times()."""
        self._stage_ev = [] if on else None
        self._stage_videos = 0

    def stage_times(self) -> dict:
        """{'videos': n, 'tower_ms': .., 'slotpool_ms': .., 'prefill_ms': ..} summed over the recorded batches (synchronises the device)"""
        torch.cuda.synchronize(self.device)
        out = {"videos": getattr(self, "_stage_videos", 0), "tower_ms": 0.0, "slotpool_ms": 0.0, "prefill_ms": 0.0}
        for kind, e0, e1 in (getattr(self, "_stage_ev", None) or []):
            out[kind + "_ms"] += e0.elapsed_time(e1)
        return out

    def _bracket(self, kind: str, fn, record: bool):
        if not record:
            return fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        self._stage_ev.append((kind, e0, e1))
        return r

    def feature_groups(self, videos: Sequence[torch.Tensor]):
        """(first, last + 1) video ranges whose ViT features (12 GB at most) one vit_forward_many call computes — encode_prefill's grouping"""
        per_frame = self.cfg.vision_patches * self.cfg.vision_hidden_size * 2
        groups, g0, B = [], 0, len(videos)
        while g0 < B:
            g1, nbytes = g0, 0
            while g1 < B and (g1 == g0 or nbytes + videos[g1].shape[0] * per_frame <= 12 << 30):
                nbytes += videos[g1].shape[0] * per_frame
                g1 += 1
            groups.append((g0, g1))
            g0 = g1
        return groups

    def encode_prefill(self, videos: Sequence[torch.Tensor], timestamps: Sequence, input_ids: Sequence[Sequence[int]], slot0: int = 0,
                       record_stages: bool = False, share_prefix: bool = True):
        """Stage 1 of generate() for a batch: CLIP tower (over the batch's frame stream) -> slot pool + time rows -> splice -> prefill
        into KV slots slot0 .. slot0 + B - 1.  Runs on the current stream; touches no decode state, so it may run on another stream
        while an earlier batch (other slots) is being decoded (generate_stream).
        A batch of share_prefix_min_batch videos or more whose prompts agree before <video> (one question for every video: the evaluation loops)
        prefills those P rows once, into the batch's first slot, and every run continues from a copy of them (trace_llm_prefill_shared): the same
        bits in every slot as whole prefills leave (16-bit KV cache and 16-bit weights only: a continuation is not bit-identical under the others).
        Returns (first slot, P) then — what decode(shared_prefix=) takes — and None otherwise.  share_prefix=False: whole prefills whatever the
        prompts (generate_queue: rows admitted later could not hold the same shared rows)."""
        B = len(videos)
        if slot0 < 0 or slot0 + B > self.max_batch:
            raise ValueError(f"slots {slot0}..{slot0 + B - 1} exceed the engine's {self.max_batch} KV slots")
        rec = bool(record_stages) and getattr(self, "_stage_ev", None) is not None
        if rec:
            self._stage_videos += B
        # prefill: runs of up to 4 neighbours whose spliced prompts have the same length share one pass (M = 4 L fills the GEMM tile grids in whole
        # rounds of the CUs); the spliced embeddings of a run wait in `held`
        held: List[torch.Tensor] = []                 # spliced embeds of slots held_slot0 .. (equal lengths)
        held_slot0 = 0
        P = 0                                         # prompt rows shared by the batch
        if share_prefix and 2 <= B and B >= self.share_prefix_min_batch and not self.kv_cache and not self.llm_fp8:
            P = shared_prefix_len(input_ids)
        if P:
            def prefix():
                self.embed_rows(input_ids[0][:P])
                self.prefill(slot0, P)
            self._bracket("prefill", prefix, rec)

        def flush():
            nonlocal held
            if held and P:
                self._bracket("prefill", lambda: self.prefill_shared(slot0, held_slot0, P, [e[P:] for e in held]), rec)
            elif len(held) == 1:
                self._bracket("prefill", lambda: self.prefill(held_slot0, held[0].shape[0], embeds=held[0]), rec)
            elif len(held) == 2:
                self._bracket("prefill", lambda: self.prefill_pair(held_slot0, held[0], held[1]), rec)
            elif held:
                self._bracket("prefill", lambda: self.prefill_multi(held_slot0, held), rec)
            held = []

        feats = None
        if B > 1 and self.vit_batch_frames > self.max_frames and self.cfg.mm_projector_type != "stc_connector":
            groups, feats = self.feature_groups(videos), {}      # the tower runs over groups of videos (whole GEMM rounds); 12 GB of features at a time
        for b in range(B):
            if feats is not None:
                if b not in feats:
                    g = next(g for g in groups if g[0] <= b < g[1])
                    feats = dict(zip(range(g[0], g[1]), self._bracket("tower", lambda: self.vit_forward_many(videos[g[0]:g[1]]), rec)))
                fb = feats.pop(b)
                if self._dbg is not None:
                    self._dbg("feats", slot0 + b, fb)
                self._bracket("slotpool", lambda: self.encode_features(fb, timestamps[b]), rec)
            else:
                self._bracket("tower", lambda: self.encode_video(videos[b], timestamps[b]), rec)      # (tower + slot pool in one call)
            if B == 1:
                L1 = self.splice(input_ids[b])
                self._bracket("prefill", lambda: self.prefill(slot0, L1), rec)
                continue
            L, emb = self.splice(input_ids[b], want_output=True)
            if held and (held[0].shape[0] != L or len(held) == self.prefill_group(held[0].shape[0] - P)):
                flush()
            if not held:
                held_slot0 = slot0 + b
            held.append(emb)
        flush()
        return (slot0, P) if P else None

    def decode(self, slots: Sequence[int], heads: Sequence[int], max_new_tokens: int, eos: int = -1, use_graph: bool = True,
               forced: Optional[Sequence[Sequence[int]]] = None, sampling: Optional[SamplingParams] = None, logprobs: bool = False,
               logits: Optional[LogitsParams] = None, shared_prefix=None, constraints: Optional[Constraints] = None, retire_finished: bool = False,
               row_params: Optional[Sequence[RowParams]] = None):
        """Stage 2 of generate(): the decode loop over prefilled KV slots, on the current stream -> (ids per sequence, final heads).
        row_params: one RowParams per row (decode_begin) whose None fields fall back to sampling= / logits= / max_new_tokens=; every row then decodes
        under its own params to its own bound.  Forced ids are refused only for a row whose processors are armed, or under constraints.
        retire_finished: every retire_chunk steps the rows whose recorded ids end in EOS or a stop sequence leave the running batch (retire_rows, when
        retire.retire_plan says it pays), so the later steps attend and project the live rows only; the result has every row, in its original order,
        shaped as with the flag off.  A row's ids, length and log-probabilities are a function of its own logits: on a decoder whose logits do not
        depend on rounding they are the flag-off ones exactly, sampled draws included; on real weights a row that decodes on in a smaller batch sees
        that batch size's rounding.  The returned head of a retired row is the one it had when it left.  Off (the default):
        today's loop, launches and graphs.  ValueError with sampling parameters outside the device sampler's domain (they run the host loop).
        constraints: bad words / suppressed ids / stop sequences (Constraints; None or all off = today's launches and graphs), inside the decode
        step like `logits` (set_constraints); not together with forced ids.
        shared_prefix: what encode_prefill returned for these slots (decode_begin: the attention reads the shared rows from one slot; same results).
        logits: repetition penalty / no-repeat n-grams / min_new_tokens (LogitsParams; None or all off = today's launches and graphs), applied
        inside the decode step to the ids each row has generated so far (set_logits_params); not together with forced ids.
        sampling: None / temperature <= 0 = greedy; otherwise every id is drawn on the device (trace_decode_set_sampling: same graphs, same
        stepping), or — parameters outside the device sampler's domain — one eager step at a time with the host statement of the same rules.
        logprobs: the result gains a third element, one float32 array per row as long as that row's ids: the log-probability of every emitted
        token under the model's own (unwarped) distribution, computed inside the decode step (trace_decode_set_logprobs)."""
        armed = logits is not None and not logits.off
        bound = constraints is not None and not constraints.off
        if row_params is not None:
            if len(row_params) != len(slots):
                raise ValueError("one RowParams per slot")
            row_params = [(r if r is not None else RowParams()).over(sampling, logits, max_new_tokens).check(max_new_tokens) for r in row_params]
            sampling, logits, armed = None, None, False               # every row carries its own from here on
        if (armed or bound) and forced is not None:
            raise ValueError("logits processors and constraints act on the ids a row has recorded; under forced ids those are not the fed ones "
                             "(forced= with logits= / constraints=)")
        if bound:
            check_constraints(constraints.stop_sequences, constraints.bad_words_ids, constraints.suppress_tokens, constraints.begin_suppress_tokens,
                              self.cfg.total_vocab)
        if sampling is not None and not sampling.greedy and not sampling.on_device:
            if retire_finished:
                raise ValueError("retire_finished=True needs the device decode loop: these sampling parameters lie outside the device sampler's "
                                 "domain and run one host-selected step at a time")
            return self.decode_stepwise(slots, heads, max_new_tokens, eos, forced, sampling, logprobs, logits, shared_prefix=shared_prefix,
                                        constraints=constraints)
        slots = list(slots)
        if len(heads) != len(slots) or (forced is not None and len(forced) != len(slots)):
            raise ValueError("one head (and forced row) per slot")
        reqs = [(None, None, s, h, None if forced is None else forced[r], None if row_params is None else row_params[r])
                for r, (s, h) in enumerate(zip(slots, heads))]
        with self._modes(sampling, logprobs, logits, constraints):
            return self._loop(iter(reqs), lambda _, rs: [r[2] for r in rs], DECODE if row_params is None else DECODE_ROWS, len(slots), max_new_tokens, eos,
                              logprobs, constraints, use_graph, retire_finished, shared_prefix).columns()

    @contextlib.contextmanager
    def _modes(self, sampling, logprobs, logits, constraints):
        """the modes of the decode batches begun inside: device sampling, log-probabilities, logits processors and constraints, each set only when
        it is on and taken down, in reverse order, whatever happens inside"""
        on_dev = sampling is not None and not sampling.greedy
        armed = logits is not None and not logits.off
        bound = constraints is not None and not constraints.off
        if on_dev:
            self.set_sampling(sampling)
        if logprobs:
            self.set_logprobs(True)
        if armed:
            self.set_logits_params(logits)
        try:
            if bound:
                self.set_constraints(constraints)
            yield
        finally:
            if bound:
                self.set_constraints(None)
            if armed:
                self.set_logits_params(None)
            if logprobs:
                self.set_logprobs(False)
            if on_dev:
                self.set_sampling(None)

    def _loop(self, requests, place, rules, cap, max_new_tokens, eos, logprobs, constraints, use_graph, retiring, shared_prefix=None) -> RowBook:
        """decode_loop.decode_loop on this engine's device primitives -> the book that holds every request's result"""
        mn = int(max_new_tokens)
        dev = Device(begin=lambda slots, heads, forced, rp: self.decode_begin(slots, heads, mn, eos, forced, shared_prefix=shared_prefix, row_params=rp),
                     admit=self._admit, steps=lambda n: self.decode_steps(n, use_graph), retire=self.retire_rows, read=self.decode_read,
                     read_logprobs=self.decode_read_logprobs)
        bound = constraints is not None and not constraints.off
        return decode_loop(dev, requests, place, RowBook(range(cap), logprobs), rules, cap=cap, max_new=mn, eos=eos,
                           constraints=constraints if bound else None, chunk=self.retire_chunk, retiring=retiring, retire_fraction=self.retire_fraction,
                           admit_fraction=self.admit_fraction)

    def decode_stepwise(self, slots: Sequence[int], heads: Sequence[int], max_new_tokens: int, eos: int = -1,
                        forced: Optional[Sequence[Sequence[int]]] = None, sampling: Optional[SamplingParams] = None, logprobs: bool = False,
                        logits: Optional[LogitsParams] = None, stopping=None, shared_prefix=None, constraints: Optional[Constraints] = None,
                        retire_finished: bool = False):
        """decode() one eager step at a time with the token picked on the host: the one loop in host-select mode (sampling parameters outside the
        device sampler's domain, stopping criteria).  Every rule is the device step's.  The row the pick reads is the processed one
        (logits_process: the history is the ids recorded so far) when `logits` is armed, else the raw one; sampled rows go through sample(),
        greedy rows take the lowest id among equal maxima of the head's range; a forced id overrides the pick; the log-probability is the fed
        token's on the raw row.  `constraints`: the ban rules ride behind the processors in the same loose-row op (logits_process_ex), and a row
        whose ids end in a stop sequence is finished as the device step finishes it (sampling.ends_stopped): it keeps the ids it held then, and the
        history its later picks see is that.  A row is finished when its recorded ids end in `eos` or `stopping` fired for it - stopping(ids per row) ->
        one bool per row, asked after every step but the last while some row is unfinished; a row it fired for keeps the ids (and log-probabilities) it held then,
        while its returned head is the whole run's: the device goes on feeding it, as it does a row past its EOS.  The greedy pick is taken on the
        device (sampling.argmax_rows: B ids come back); the recorded ids are read back after every step, since both finished rules look at them.  The
        loop ends when every row is finished or max_new_tokens ids were fed.  Returns what decode() returns.
        retire_finished=True is a ValueError: host-select mode has no step graph and trace_decode_retire does not serve it."""
        if retire_finished:
            raise ValueError("retire_finished=True needs the device decode loop; decode_stepwise runs in host-select mode")
        B, cfg = len(slots), self.cfg
        greedy = sampling is None or sampling.greedy
        armed = logits is not None and not logits.off
        bound = constraints is not None and not constraints.off
        if bound and forced is not None:
            raise ValueError("constraints act on the ids a row has recorded; under forced ids those are not the fed ones (forced= with constraints=)")
        self.host_mode(True)
        try:
            raw = self.decode_begin(list(slots), heads, max_new_tokens, eos, forced, want_logits=True, shared_prefix=shared_prefix)
            ids, cur = [[] for _ in range(B)], list(heads)
            lp = np.zeros((B, max_new_tokens), np.float32)
            stopped = [None] * B                          # the length at which `stopping` fired for the row
            for step in range(max_new_tokens):
                if bound:
                    hist = [x if n is None else x[:n] for x, n in zip(ids, stopped)]
                    rows = self.logits_process_ex(raw, cur, hist, logits, [step] * B, eos, constraints)
                else:
                    rows = self.logits_process(raw, cur, ids, logits, [step] * B, eos) if armed else raw
                if greedy:
                    tok = argmax_rows(rows, cur, cfg.vocab_size, cfg.time_vocab_size, cfg.score_vocab_size)
                else:
                    tok = self.sample(rows, cur, sampling, [step] * B)
                if forced is not None:
                    tok = [f[step] if step < len(f) and f[step] >= 0 else t for t, f in zip(tok, forced)]
                val = self.token_logprob(raw, cur, tok) if logprobs else None       # under the head the token was picked from
                self.feed(tok)
                ids, cur = self.decode_read()
                if logprobs:
                    for b in range(B):
                        if len(ids[b]) == step + 1:
                            lp[b, step] = val[b]
                if bound:                                 # (the device records on in host-select mode: the length at which the stop rule fired is kept here)
                    stopped = [len(x) if n is None and ends_stopped(x, -1, constraints) else n for x, n in zip(ids, stopped)]
                if step == max_new_tokens - 1:
                    break
                done = [ends_stopped(x, eos) for x in ids]
                if stopping is not None and not all(done):
                    stopped = [len(x) if n is None and f else n for x, n, f in zip(ids, stopped, stopping(ids))]
                if all(d or n is not None for d, n in zip(done, stopped)):
                    break
                raw = self.decode_steps(1, use_graph=False, want_logits=True)
            ids = [x if n is None else x[:n] for x, n in zip(ids, stopped)]
            return (ids, cur, [lp[b, : len(x)].copy() for b, x in enumerate(ids)]) if logprobs else (ids, cur)
        finally:
            self.host_mode(False)

    def generate(self, videos: Sequence[torch.Tensor], timestamps: Sequence, input_ids: Sequence[Sequence[int]],
                 heads: Sequence[int], max_new_tokens: int, eos: int = -1, use_graph: bool = True,
                 forced: Optional[Sequence[Sequence[int]]] = None, sampling: Optional[SamplingParams] = None, logprobs: bool = False,
                 logits: Optional[LogitsParams] = None, constraints: Optional[Constraints] = None, retire_finished: bool = False):
        B = len(videos)
        if B > self.decode_batch_max:
            raise ValueError(f"batch {B} exceeds the engine's decode batch {self.decode_batch_max}")
        shared = self.encode_prefill(videos, timestamps, input_ids, 0, record_stages=True)
        return self.decode(range(B), heads, max_new_tokens, eos, use_graph, forced, sampling, logprobs=logprobs, logits=logits, shared_prefix=shared,
                           constraints=constraints, retire_finished=retire_finished)

    def generate_queue(self, requests: Iterable, max_new_tokens: int, eos: int = -1, *, max_rows: Optional[int] = None,
                       sampling: Optional[SamplingParams] = None, logprobs: bool = False, logits: Optional[LogitsParams] = None,
                       constraints: Optional[Constraints] = None, use_graph: bool = True, per_request: bool = False):
        """Continuous batching: requests (video, timestamps, input_ids, head[, forced ids]) flow through one running decode batch of at most
        max_rows rows (default and bound: decode_batch_max) -> one (ids, head[, logprobs]) per request, in request order.  The first max_rows
        requests are encoded, prefilled (whole prefills: no shared prefix) and begun as a batch; every retire_chunk steps the recorded ids are read,
        the rows that ended (EOS, a stop sequence, or max_new_tokens ids) leave (retire_rows, by retire.retire_plan), and once admit.admit_plan says
        the room is worth it the next requests are encoded and prefilled into the KV slots the retired rows freed and appended to the batch
        (admit_rows); the boundary then looks again, so a row whose token 0 already ends it leaves before it has ridden a chunk.  When every row of
        the batch has ended at once, the next requests begin a batch of their own.  KV slot and batch position are independent: the book holds the
        map and the free slots.  Everything runs on the current stream; the admitted rows' encode and prefill do not
        overlap the decode (generate_stream's banks do that for whole batches).
        A row's ids, length and log-probabilities are a function of its own logits, its own step count and (sampled) its Philox row index, which is its
        request index counted from the first request of the batch it joined: on a decoder whose logits do not depend on rounding they are those of
        generate() of the request alone, exactly; on real weights a row sees the rounding of the batch sizes it is decoded in.
        max_new_tokens, eos, sampling, logits and constraints hold for every request, unless per_request=True: a request may then carry a sixth element,
        a RowParams (forced ids or None in the fifth), whose None fields fall back to the call's sampling / logits / max_new_tokens — the latter stays the
        bound of every row's and the stride; a request's own seed applies to its row, at the same Philox row index; a row leaves at its own bound and
        the chunk is as long as the longest remainder of a live row.  eos, constraints and logprobs stay the call's.  With per_request=False a
        six-element request is a ValueError, found as the forced-ids one below is.  ValueError, before any work, for sampling parameters outside
        the device sampler's domain.  ValueError for a request that carries forced ids while logits= / constraints= are armed: before any work when
        `requests` is a list or a tuple (every request is looked at first); an iterator is looked at as it is pulled, so there the error comes when
        the bad request is reached — the requests before it have been decoded by then, their results are lost with the call, and the batch that
        was running is dropped (the next decode_begin starts afresh; the armed modes are taken down as after any call)."""
        def prefill_into(slots, reqs):
            i = 0
            while i < len(slots):                     # runs of neighbouring slots go through encode_prefill together (it pairs equal-length prompts)
                j = i + 1
                while j < len(slots) and slots[j] == slots[j - 1] + 1:
                    j += 1
                self.encode_prefill([r[0] for r in reqs[i:j]], [r[1] for r in reqs[i:j]], [list(r[2]) for r in reqs[i:j]], slots[i],
                                    record_stages=True, share_prefix=False)
                i = j
            return slots

        return self._serve_queue(requests, prefill_into, max_new_tokens, eos, max_rows, sampling, logprobs, logits, constraints, use_graph, per_request)

    def decode_queue(self, slots: Sequence[int], heads: Sequence[int], max_new_tokens: int, eos: int = -1, *, max_rows: Optional[int] = None,
                     forced: Optional[Sequence[Sequence[int]]] = None, sampling: Optional[SamplingParams] = None, logprobs: bool = False,
                     logits: Optional[LogitsParams] = None, constraints: Optional[Constraints] = None, use_graph: bool = True,
                     row_params: Optional[Sequence[Optional[RowParams]]] = None):
        """generate_queue's decode side alone, over KV slots that are prefilled already (what decode() is to generate()): request r decodes slot
        slots[r] from head heads[r]; at most max_rows of them run together -> one (ids, head[, logprobs]) per slot, in the order given.  No slot
        is recycled: every request keeps its own.  row_params: one RowParams (or None) per slot = generate_queue(per_request=True)."""
        slots = [int(s) for s in slots]
        if len(set(slots)) != len(slots) or len(heads) != len(slots) or (forced is not None and len(forced) != len(slots)) or \
                (row_params is not None and len(row_params) != len(slots)):
            raise ValueError("one head (forced row, RowParams) per slot, every slot once")
        reqs = [(None, None, s, int(h), None if forced is None else forced[r]) + (() if row_params is None else (row_params[r],))
                for r, (s, h) in enumerate(zip(slots, heads))]
        return self._serve_queue(reqs, lambda _, rs: [r[2] for r in rs], max_new_tokens, eos, max_rows, sampling, logprobs, logits, constraints, use_graph,
                                 row_params is not None)

    def _serve_queue(self, requests, place, max_new_tokens, eos, max_rows, sampling, logprobs, logits, constraints, use_graph, per_request):
        """generate_queue / decode_queue: the requests are checked (decode_loop.checked_requests: a list whole and before any work, an iterator as it
        is pulled), the modes armed and the loop run.  place(slots the book hands out, requests) -> the KV slots the rows decode from, prefilled"""
        requests = checked_requests(requests, max_new_tokens, self.cfg.total_vocab, sampling, logits, constraints, per_request)
        cap = max(1, min(int(max_rows) if max_rows else self.decode_batch_max, self.decode_batch_max, self.max_batch))
        if per_request:
            sampling = logits = None                   # a per-row batch ignores the batch-wide sampling and logits params: nothing to set or take down
        with self._modes(sampling, logprobs, logits, constraints):
            return self._loop(requests, place, QUEUE, cap, max_new_tokens, eos, logprobs, constraints, use_graph, True).results()

    def generate_samples(self, video: torch.Tensor, timestamps, prompt_ids: Sequence[int], head: int, n: int, max_new_tokens: int, eos: int = -1,
                         sampling: Optional[SamplingParams] = None, use_graph: bool = True, logits: Optional[LogitsParams] = None,
                         constraints: Optional[Constraints] = None, retire_finished: bool = False):
        """n sampled continuations of ONE prompt from one tower pass and one prefill: the prompt is encoded and prefilled into KV slot 0, its rows
        are copied to slots 1 .. n - 1 (kv_copy), and slots 0 .. n - 1 decode as one batch with log-probabilities on.  Row r draws with Philox
        row index r, as any decode batch does, so the result equals generate() of the prompt repeated n times with the same SamplingParams:
        (ids, heads, logprobs), rows in decode order."""
        if n < 1 or n > min(self.max_batch, self.decode_batch_max):
            raise ValueError(f"n = {n} must lie in [1, {min(self.max_batch, self.decode_batch_max)}] (the engine's KV slots / decode batch)")
        if sampling is None or sampling.greedy:
            raise ValueError("generate_samples needs sampling parameters with temperature > 0: greedy rows would all be identical")
        self.encode_video(video, timestamps)
        L = self.splice(list(prompt_ids))
        self.prefill(0, L)
        if n > 1:
            self.kv_copy(0, list(range(1, n)), L)
        return self.decode(range(n), [int(head)] * n, max_new_tokens, eos, use_graph, None, sampling, logprobs=True, logits=logits, constraints=constraints,
                           retire_finished=retire_finished)

    def generate_questions(self, video: torch.Tensor, timestamps, prompts: Sequence[Sequence[int]], heads: Sequence[int], max_new_tokens: int,
                           eos: int = -1, sampling: Optional[SamplingParams] = None, use_graph: bool = True,
                           forced: Optional[Sequence[Sequence[int]]] = None, prefix_key=None, logprobs: bool = False,
                           logits: Optional[LogitsParams] = None, constraints: Optional[Constraints] = None, retire_finished: bool = False):
        """generate() for Q prompts about ONE video whose ids agree up to and including the <video> placeholder (the reference's per-question
        loops, trace/eval/videomme/evaluate.py:349-386): the tower, the slot pool and the prefill of the common prefix run once (slot 0), the
        prefix's KV rows are copied to the other Q - 1 slots, each prompt's rows after <video> are appended (one pass per group of equal
        length, at most 8 prompts each, over consecutive slots), and all Q rows decode as one batch — row q is prompt q, as in generate().
        Returns what generate() returns, bit-identical to it.  prefix_key: recorded with set_prefix_entry() once slot 0 holds the shared rows."""
        Q = len(prompts)
        if Q > min(self.max_batch, self.decode_batch_max):
            raise ValueError(f"{Q} prompts exceed the engine's KV slots / decode batch ({self.max_batch} / {self.decode_batch_max})")
        if len(heads) != Q:
            raise ValueError("one head per prompt")
        prefix, suffixes = split_questions(prompts)
        if any(len(x) == 0 for x in suffixes):
            raise ValueError("a prompt ends at its video placeholder: nothing to append (use generate())")
        groups = group_by_length([len(x) for x in suffixes])
        self.encode_video(video, timestamps)
        P = self.splice(prefix)
        self.prefill(0, P)
        if Q > 1:
            self.kv_copy(0, list(range(1, Q)), P)
        slot_of, slot = [0] * Q, 0
        for n_rows, idx in groups:
            cap = max(1, self.prefill_rows // n_rows)          # a run of long suffixes must also fit the prefill workspaces
            for o in range(0, len(idx), cap):
                run = idx[o:o + cap]
                self.prefill_append(slot, P, [self.embed_rows(suffixes[i], want_output=True) for i in run])
                for i in run:
                    slot_of[i] = slot
                    slot += 1
        if prefix_key is not None:
            self.set_prefix_entry(prefix_key, P)
        return self.decode(slot_of, heads, max_new_tokens, eos, use_graph, forced, sampling, logprobs=logprobs, logits=logits, constraints=constraints,
                           retire_finished=retire_finished)

    # ---- two-stage pipeline over a stream of batches ---------------------------------------------------
    def make_streams(self, decode_cus: int = 0):
        """The pipeline's (encode stream, decode stream).  decode_cus > 0 confines the decode stream to that many CUs and the encode
        stream to the rest (trace_stream_create: CU-masked HIP streams, spread evenly over the 8 XCDs; the persistent GEMM's grid on such a
        stream is capped at the stream's CU count): the MFMA-bound GEMMs
        and the HBM-bound decode kernels then run side by side instead of taking turns on the whole chip."""
        if decode_cus <= 0:
            return torch.cuda.Stream(self.device), torch.cuda.Stream(self.device)
        ncu = torch.cuda.get_device_properties(self.device).multi_processor_count
        if decode_cus % 8 or decode_cus >= ncu:
            raise ValueError("decode_cus must be a multiple of 8 (the XCD count) below the CU count")
        def masked(lo, n):
            h = C.c_void_p()
            _lib.check(self.lib.trace_stream_create(self.h, lo, n, C.byref(h)))
            return torch.cuda.ExternalStream(h.value, device=self.device)
        dec, enc = masked(0, decode_cus), masked(decode_cus, ncu - decode_cus)      # (trace_stream_create caps each stream's persistent GEMMs at its CU count)
        return enc, dec

    def generate_stream(self, batches: Iterable, max_new_tokens: int, eos: int = -1, use_graph: bool = True, streams=None,
                        sampling: Optional[SamplingParams] = None, logprobs: bool = False, logits: Optional[LogitsParams] = None,
                        constraints: Optional[Constraints] = None, retire_finished: bool = False):
        """generate() over a stream of batches as a two-stage pipeline: while batch k decodes (HBM-bound) on one stream, batch k+1
        runs its ViT + slot pool + prefill (MFMA-bound) on another, into the other half of the KV slots.  `batches` yields
        (videos, timestamps, input_ids, heads, forced-or-None); yields generate()'s result per batch, in order.  Every batch holds at
        most max_batch // 2 videos.  sampling / logits / constraints: as decode(), the same params (and seed) for every batch; retire_finished: as decode(), for every batch.  Results are identical to generate() batch by batch: the stages share no buffers (KV banks,
        prefill / ViT scratch vs decode scratch) and every kernel's reductions have a fixed order.

        The decode stage is issued from a worker thread: one decode batch is ~75 k kernel dispatches, far more than a HIP stream's
        queue holds, so the issuing thread blocks until the GPU has consumed most of them — issued from the caller's thread it would
        hold back the encode stage's launches and the two stages would run one after the other (profiles/r03_overlap_probe_single_thread.jsonl)."""
        import concurrent.futures as cf
        half = self.max_batch // 2
        if half < 1:
            raise ValueError("generate_stream needs an engine with max_batch >= 2 (two banks of KV slots)")
        enc_s, dec_s = streams if streams is not None else self.make_streams()
        cur = torch.cuda.current_stream(self.device)
        enc_s.wait_stream(cur); dec_s.wait_stream(cur)

        def dec_job(bank, heads, forced, B, ready, shared):
            torch.cuda.set_device(self.device)
            with torch.cuda.stream(dec_s):
                dec_s.wait_event(ready)
                # (logprobs: read inside this job, right after the ids — decode() returns them, nothing goes through engine state afterwards)
                return self.decode(range(bank * half, bank * half + B), heads, max_new_tokens, eos, use_graph, forced, sampling, logprobs=logprobs,
                                   logits=logits, shared_prefix=shared, constraints=constraints, retire_finished=retire_finished)

        pending = None                                  # (bank, heads, forced, B, ready event, shared prefix): prefilled, waiting for its decode
        bank = 0
        # profiling mode 2 brackets single launches with HIP events: meaningful only while a stage has the GPU to itself — the first batch's
        # encode (pipeline fill) and the last batch's decode (drain); in between the brackets are off
        brackets = lambda m: _lib.check(self.lib.trace_set_profile_brackets(self.h, m))
        try:                                            # whatever ends the generator (exhaustion, an exception, the caller closing it early): both brackets back on
            with cf.ThreadPoolExecutor(max_workers=1, thread_name_prefix="trace-decode") as pool:
                for item in batches:
                    videos, timestamps, input_ids, heads, forced = item
                    if len(videos) > min(half, self.decode_batch_max):
                        raise ValueError(f"batch of {len(videos)} exceeds max_batch // 2 = {half} (two KV banks)")
                    brackets(1 if pending is None else 0)
                    fut = pool.submit(dec_job, *pending) if pending is not None else None
                    enc_s.wait_stream(cur)                  # the batch's frames may have been made on the caller's stream (device preprocessing)
                    try:
                        with torch.cuda.stream(enc_s):
                            shared = self.encode_prefill(videos, timestamps, input_ids, bank * half, record_stages=pending is None)      # (the bank's own shared slot)
                            if self._dbg is not None:
                                self._dbg("prefilled", bank * half, None)
                            ready = torch.cuda.Event()
                            ready.record(enc_s)
                    finally:
                        out = fut.result() if fut is not None else None      # also drains the decode stage before an exception propagates
                    if out is not None:
                        yield out
                    pending = (bank, list(heads), forced, len(videos), ready, shared)
                    bank ^= 1
                if pending is not None:
                    brackets(2)
                    out = pool.submit(dec_job, *pending).result()
                    cur.wait_stream(dec_s); cur.wait_stream(enc_s)
                    yield out
        finally:
            brackets(3)


def _hist_tensors(hist, B, dev):
    """one history per row -> (int32 [B, ld] device, ld, int32 [B] lengths device)"""
    if len(hist) != B:
        raise ValueError("one history per row")
    ldh = max(1, max(len(h) for h in hist))
    hh = torch.tensor([[int(t) for t in h] + [0] * (ldh - len(h)) for h in hist], dtype=torch.int32, device=dev)
    return hh, ldh, torch.tensor([len(h) for h in hist], dtype=torch.int32, device=dev)


def constraints_c(constraints: Constraints, n_vocab):
    """(trace_constraints for the C ABI, the numpy arrays its pointers look into - keep them until the call has returned); ValueError first"""
    check_constraints(constraints.stop_sequences, constraints.bad_words_ids, constraints.suppress_tokens, constraints.begin_suppress_tokens, n_vocab)

    def csr(seqs):
        off = np.cumsum([0] + [len(w) for w in seqs], dtype=np.int64).astype(np.int32)
        return off, np.array([t for w in seqs for t in w], dtype=np.int32)
    so, si = csr(constraints.stop_sequences)
    bo, bi = csr(constraints.bad_words_ids)
    su, bg = np.array(constraints.suppress_tokens, dtype=np.int32), np.array(constraints.begin_suppress_tokens, dtype=np.int32)
    keep = (so, si, bo, bi, su, bg)
    ptr = lambda a: a.ctypes.data if a.size else None
    k = _lib.TraceConstraintsC(C.sizeof(_lib.TraceConstraintsC), len(constraints.stop_sequences), len(constraints.bad_words_ids), len(su), len(bg),
                               ptr(so), ptr(si), ptr(bo), ptr(bi), ptr(su), ptr(bg))
    return k, keep


def sampling_c(sampling: SamplingParams):
    """trace_sampling for the C ABI (trace_decode_set_sampling_ex / trace_op_sample_ex)"""
    return _lib.TraceSamplingC(C.sizeof(_lib.TraceSamplingC), float(sampling.temperature), int(sampling.top_k), float(sampling.top_p), int(sampling.seed),
                               float(sampling.min_p), float(sampling.typical_p), float(sampling.epsilon_cutoff), float(sampling.eta_cutoff))


def row_params_c(rows: Sequence[RowParams], max_new: int):
    """trace_row_params [len(rows)] for the C ABI (trace_decode_set_row_params / trace_decode_admit_ex), every row checked (RowParams.check) first;
    a None max_new_tokens is the batch's"""
    arr = (_lib.TraceRowParamsC * len(rows))()
    for i, r in enumerate(rows):
        r = (r if r is not None else RowParams()).check(max_new)
        sp = r.sampling if r.sampling is not None and not r.sampling.greedy else SamplingParams(temperature=0.0)
        lp = r.logits if r.logits is not None else LogitsParams()
        arr[i] = _lib.TraceRowParamsC(C.sizeof(_lib.TraceRowParamsC), sampling_c(sp), float(lp.repetition_penalty), int(lp.no_repeat_ngram_size),
                                      int(lp.min_new_tokens), int(r.max_new_tokens if r.max_new_tokens is not None else max_new))
    return arr


# ---- kernel-level wrappers for unit tests / microbenchmarks -------------------------------------
class ops:
    element = "bf16"               # which library the wrappers call: "bf16" (libtrace_hip.so) or "f16" (libtrace_hip_f16.so); ops.use()

    @staticmethod
    def use(element: str):
        _lib.load(element)
        ops.element = element

    @staticmethod
    def dtype() -> torch.dtype:
        return torch.float16 if ops.element == "f16" else torch.bfloat16

    @staticmethod
    def sample(logits, heads, sampling: SamplingParams, steps, V: int, Tv: int, Sv: int, element=None):
        """trace_op_sample_ex: logits [B, ld >= V+1+Tv+Sv] fp32 (device) -> int32 ids [B] (device), row b drawn from head heads[b] with Philox step
        steps[b] and row index b.  heads / steps: sequences of ints or int32 device tensors."""
        lib = _lib.load(element or ops.element)
        lg = logits.contiguous()
        B, ld = lg.shape
        dev = lg.device
        hd = heads if isinstance(heads, torch.Tensor) else torch.tensor([int(h) for h in heads], dtype=torch.int32, device=dev)
        st = steps if isinstance(steps, torch.Tensor) else torch.tensor([int(x) for x in steps], dtype=torch.int32, device=dev)
        out = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.check(lib.trace_op_sample_ex(_ptr(lg), ld, B, _ptr(hd), V, Tv, Sv, C.byref(sampling_c(sampling)), _ptr(st), _ptr(out), _stream()))
        return out

    @staticmethod
    def logits_process(logits, heads, hist, params: LogitsParams, steps, eos: int, V: int, Tv: int, Sv: int, element=None):
        """trace_op_logits_process: logits [B, ld >= V+1+Tv+Sv] fp32 (device) -> a new fp32 [B, ld] (device): row b under head heads[b] with the
        repetition penalty, the n-gram bans and the min_new_tokens rule of `params` for history hist[b] (a sequence of id sequences, any lengths)
        at device step steps[b]; -inf outside the head.  sampling.process_row_ref bit for bit.  heads / steps: sequences of ints or int32 device tensors."""
        lib = _lib.load(element or ops.element)
        lg = logits.contiguous()
        B, ld = lg.shape
        dev = lg.device
        hd = heads if isinstance(heads, torch.Tensor) else torch.tensor([int(h) for h in heads], dtype=torch.int32, device=dev)
        st = steps if isinstance(steps, torch.Tensor) else torch.tensor([int(x) for x in steps], dtype=torch.int32, device=dev)
        if len(hist) != B:
            raise ValueError("one history per row")
        ldh = max(1, max(len(h) for h in hist))
        hh = torch.tensor([[int(t) for t in h] + [0] * (ldh - len(h)) for h in hist], dtype=torch.int32, device=dev)
        hl = torch.tensor([len(h) for h in hist], dtype=torch.int32, device=dev)
        out = torch.empty_like(lg) if ld == V + 1 + Tv + Sv else torch.full_like(lg, float("-inf"))      # (the op writes columns [0, V+1+Tv+Sv))
        _lib.check(lib.trace_op_logits_process(_ptr(lg), ld, B, _ptr(hd), V, Tv, Sv, _ptr(hh), ldh, _ptr(hl), _ptr(st), int(eos),
                                               float(params.repetition_penalty), int(params.no_repeat_ngram_size), int(params.min_new_tokens),
                                               _ptr(out), _stream()))
        return out

    @staticmethod
    def logits_process_ex(logits, heads, hist, params: Optional[LogitsParams], steps, eos: int, constraints: Optional[Constraints], V: int, Tv: int,
                          Sv: int, element=None):
        """trace_op_logits_process_ex: ops.logits_process (params None = all three off) with the ban rules of `constraints` (None = none) behind
        the processors - bad words, suppress, begin-suppress, min_new_tokens over every stop sequence of one id: sampling.constrain_row_ref of
        sampling.process_row_ref, bit for bit.  ValueError for ids outside [0, V+1+Tv+Sv) or lists beyond the device's bounds."""
        lib = _lib.load(element or ops.element)
        params = params if params is not None else LogitsParams()
        lg = logits.contiguous()
        B, ld = lg.shape
        dev = lg.device
        hd = heads if isinstance(heads, torch.Tensor) else torch.tensor([int(h) for h in heads], dtype=torch.int32, device=dev)
        st = steps if isinstance(steps, torch.Tensor) else torch.tensor([int(x) for x in steps], dtype=torch.int32, device=dev)
        hh, ldh, hl = _hist_tensors(hist, B, dev)
        k, keep = (None, None) if constraints is None or constraints.off else constraints_c(constraints, V + 1 + Tv + Sv)
        out = torch.empty_like(lg) if ld == V + 1 + Tv + Sv else torch.full_like(lg, float("-inf"))      # (the op writes columns [0, V+1+Tv+Sv))
        _lib.check(lib.trace_op_logits_process_ex(_ptr(lg), ld, B, _ptr(hd), V, Tv, Sv, _ptr(hh), ldh, _ptr(hl), _ptr(st), int(eos),
                                                  float(params.repetition_penalty), int(params.no_repeat_ngram_size), int(params.min_new_tokens),
                                                  None if k is None else C.byref(k), _ptr(out), _stream()))
        del keep
        return out

    @staticmethod
    def stop_match(hist, constraints: Constraints, element=None):
        """trace_op_stop_match: one history per row (a sequence of id sequences, any lengths) -> int32 [B] (device): 1 where a stop sequence of
        `constraints` equals the last ids of the row's history (sampling.stop_match_ref), else 0."""
        lib = _lib.load(element or ops.element)
        dev = torch.device("cuda", torch.cuda.current_device())
        B = len(hist)
        hh, ldh, hl = _hist_tensors(hist, B, dev)
        k, keep = constraints_c(constraints, None)
        out = torch.empty(B, dtype=torch.int32, device=dev)
        _lib.check(lib.trace_op_stop_match(_ptr(hh), ldh, _ptr(hl), B, C.byref(k), _ptr(out), _stream()))
        del keep
        return out

    @staticmethod
    def token_logprob(logits, heads, ids, V: int, Tv: int, Sv: int, element=None):
        """trace_op_token_logprob: logits [B, ld >= V+1+Tv+Sv] fp32 (device) -> fp32 [B] (device): log softmax of row b over head heads[b]'s id
        range at ids[b] (-inf outside the range), sampling.token_logprob_ref bit for bit.  heads / ids: sequences of ints or int32 device tensors."""
        lib = _lib.load(element or ops.element)
        lg = logits.contiguous()
        B, ld = lg.shape
        dev = lg.device
        hd = heads if isinstance(heads, torch.Tensor) else torch.tensor([int(h) for h in heads], dtype=torch.int32, device=dev)
        ii = ids if isinstance(ids, torch.Tensor) else torch.tensor([int(x) for x in ids], dtype=torch.int32, device=dev)
        out = torch.empty(B, dtype=torch.float32, device=dev)
        _lib.check(lib.trace_op_token_logprob(_ptr(lg), ld, B, _ptr(hd), V, Tv, Sv, _ptr(ii), _ptr(out), _stream()))
        return out

    @staticmethod
    def score_tile(element=None) -> int:
        return _lib.load(element or ops.element).trace_op_score_tile()

    @staticmethod
    def score_rows(hidden, W, heads, ids, V: int, Tv: int, Sv: int, element=None):
        """trace_op_score_rows: hidden [R, K], W [V+1+Tv+Sv, K] (the element type, device) -> fp32 [R] (device): the log-probability of ids[r] under
        head heads[r], sampling.score_logprob_ref bit for bit given the same fp32 logits; id -1 -> 0.0, outside the head -> -inf."""
        lib = _lib.load(element or ops.element)
        x, w = hidden.contiguous(), W.contiguous()
        R, K = x.shape
        dev = x.device
        hd = heads if isinstance(heads, torch.Tensor) else torch.tensor([int(h) for h in heads], dtype=torch.int32, device=dev)
        ii = ids if isinstance(ids, torch.Tensor) else torch.tensor([int(t) for t in ids], dtype=torch.int32, device=dev)
        nbytes = int(lib.trace_op_score_ws_bytes(R, V, Tv, Sv))          # an int64: a negative status is not raised by the binding's errcheck
        if nbytes < 0:
            msg = lib.trace_last_error()
            raise _lib.TraceHipError(f"error {nbytes} in trace_op_score_ws_bytes: {msg.decode() if msg else '?'}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(R, dtype=torch.float32, device=dev)
        _lib.check(lib.trace_op_score_rows(_ptr(x), K, _ptr(w), K, K, R, _ptr(hd), _ptr(ii), V, Tv, Sv, _ptr(ws), _ptr(out), _stream()))
        return out

    @staticmethod
    def set_gemm_variant(v: int):
        _lib.check(_lib.load(ops.element).trace_op_set_gemm_variant(v))

    @staticmethod
    def tuning_names() -> List[str]:
        """the names of the library's tuning table (csrc/engine.hip TUNE_ROWS), e.g. "gemm.kernel" """
        lib, names = _lib.load(ops.element), []
        while (n := lib.trace_op_tuning_name(len(names))) is not None:
            names.append(n.decode())
        return names

    @staticmethod
    def tune(name: str, value: int):
        """sets one tuning value by its dotted name; not while launches are in flight"""
        _lib.check(_lib.load(ops.element).trace_op_tuning_set(name.encode(), int(value)))

    @staticmethod
    @contextlib.contextmanager
    def tuned(**values):
        """`with ops.tuned(gemm__kernel=8, gemm__w4__opt=1):` sets tuning values (a double underscore stands for the dot) and, on exit, restores the
        values it found — on the library of ops.element at entry."""
        element = ops.element
        lib = _lib.load(element)
        found = {}
        try:
            for key, value in values.items():
                name = key.replace("__", ".")
                v = C.c_int(0)
                _lib.check(lib.trace_op_tuning_get(name.encode(), C.byref(v)))
                found.setdefault(name, v.value)
                _lib.check(lib.trace_op_tuning_set(name.encode(), int(value)))
            yield
        finally:
            for name, value in found.items():
                _lib.check(lib.trace_op_tuning_set(name.encode(), value))

    @staticmethod
    def gemm(A, W, bias=None, R=None, epilogue=EPI_NONE, out=None, ldc=None, out_offset=0):
        """trace_op_gemm.  A [M, K], W [N, K] and R [M, No] may be strided views (unit column stride): a view's row stride is the leading dimension the
        kernel gets, its storage offset the base pointer's.  `out`: where to store instead of a fresh [M, No] tensor — a 2-D view [M, No] (ldc = its row
        stride; R itself for the in-place residual), or a flat buffer with `ldc` and `out_offset` (elements: C[m, n] = out[out_offset + m ldc + n]).
        Returns the [M, No] window that was written."""
        lib = _lib.load(ops.element)
        M, K = A.shape
        N = W.shape[0]
        No = N // 2 if epilogue == EPI_SWIGLU else N
        for t in (A, W) + (() if R is None else (R,)):
            if t.dim() != 2 or t.stride(1) != 1:
                raise ValueError("operands must be 2-D with unit column stride")
        if out is None:
            if ldc is not None or out_offset:
                raise ValueError("ldc / out_offset describe `out`")
            Cc = torch.empty((M, No), dtype=ops.dtype(), device=A.device)
        else:
            if out.dtype != ops.dtype() or out.device != A.device:
                raise ValueError("out: wrong element type or device")
            if out.dim() == 2 and ldc is None and not out_offset:
                if tuple(out.shape) != (M, No) or out.stride(1) != 1:
                    raise ValueError(f"out: expected a [{M}, {No}] view with unit column stride")
                Cc = out
            elif out.dim() == 1 and out.is_contiguous() and ldc is not None and ldc >= No and out_offset >= 0:
                if out_offset + (M - 1) * ldc + No > out.numel():
                    raise ValueError("out: the window leaves the buffer")
                Cc = out.as_strided((M, No), (ldc, 1), out.storage_offset() + out_offset)
            else:
                raise ValueError("out: a 2-D view, or a flat buffer with ldc (>= the output width) and out_offset")
        _lib.check(lib.trace_op_gemm(_ptr(A), A.stride(0), _ptr(W), W.stride(0), _ptr(Cc), Cc.stride(0), _ptr(bias), _ptr(R),
                                     0 if R is None else R.stride(0), M, N, K, epilogue, _stream()))
        return Cc

    @staticmethod
    def layernorm(x, w, b, eps):
        lib = _lib.load(ops.element)
        y = torch.empty_like(x)
        _lib.check(lib.trace_op_layernorm(_ptr(x), _ptr(y), _ptr(w), _ptr(b), x.shape[0], x.shape[1], eps, _stream()))
        return y

    @staticmethod
    def rmsnorm(x, w, eps):
        lib = _lib.load(ops.element)
        y = torch.empty_like(x)
        _lib.check(lib.trace_op_rmsnorm(_ptr(x), _ptr(y), _ptr(w), x.shape[0], x.shape[1], eps, _stream()))
        return y

    @staticmethod
    def _rows2d(t, name):
        if t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"{name}: a 2-D tensor or view with unit column stride")
        return t

    @staticmethod
    def layernorm_ex(x, w, b, eps, out=None, silu=False, res=None):
        """trace_op_layernorm_ex.  x [rows, D], `out` and `res` may be strided views (unit column stride; a view's row stride is the leading dimension
        the kernel gets); out=None: a fresh contiguous tensor; out may be x (in place) or res.  Returns the window written."""
        lib = _lib.load(ops.element)
        ops._rows2d(x, "x")
        y = torch.empty(tuple(x.shape), dtype=x.dtype, device=x.device) if out is None else ops._rows2d(out, "out")
        if tuple(y.shape) != tuple(x.shape) or (res is not None and tuple(ops._rows2d(res, "res").shape) != tuple(x.shape)):
            raise ValueError("out / res: the shape of x")
        _lib.check(lib.trace_op_layernorm_ex(_ptr(x), x.stride(0), _ptr(y), y.stride(0), _ptr(w), _ptr(b), x.shape[0], x.shape[1], float(eps),
                                             int(bool(silu)), _ptr(res), 0 if res is None else res.stride(0), _stream()))
        return y

    @staticmethod
    def rmsnorm_ex(x, w, eps, out=None):
        """trace_op_rmsnorm_ex: as layernorm_ex, without bias, SiLU or residual"""
        lib = _lib.load(ops.element)
        ops._rows2d(x, "x")
        y = torch.empty(tuple(x.shape), dtype=x.dtype, device=x.device) if out is None else ops._rows2d(out, "out")
        if tuple(y.shape) != tuple(x.shape):
            raise ValueError("out: the shape of x")
        _lib.check(lib.trace_op_rmsnorm_ex(_ptr(x), x.stride(0), _ptr(y), y.stride(0), _ptr(w), x.shape[0], x.shape[1], float(eps), _stream()))
        return y

    # ---- the STC connector's row kernels (trace_hip.h: "The STC connector's row kernels, each alone") ----
    # Tensors are contiguous and of the element type; the extents come from their shapes unless `dims` gives them (a test of the op's own refusals
    # passes extents the tensors do not have: the op answers TRACE_ERR_ARG before it touches anything).
    @staticmethod
    def _stc(*tensors):
        for t in tensors:
            if t is not None and (not t.is_contiguous() or t.dtype != ops.dtype()):
                raise ValueError("STC row ops: contiguous tensors of the element type")
        return _lib.load(ops.element)

    @staticmethod
    def dwconv3x3(x, w, out=None, dims=None):
        """trace_op_dwconv3x3: x [N, H, W, C], w [C, 9] (or [C, 1, 3, 3]) -> y [N, H, W, C] (`out`: where to store)"""
        y = torch.empty_like(x) if out is None else out
        lib = ops._stc(x, w, y)
        N, H, W, Cn = x.shape if dims is None else dims
        _lib.check(lib.trace_op_dwconv3x3(_ptr(x), _ptr(w), _ptr(y), int(N), int(H), int(W), int(Cn), _stream()))
        return y

    @staticmethod
    def avgpool(x, out=None, dims=None):
        """trace_op_avgpool: x [N, HW, C] -> y [N, C]"""
        y = torch.empty((x.shape[0], x.shape[-1]), dtype=x.dtype, device=x.device) if out is None else out
        lib = ops._stc(x, y)
        N, HW, Cn = x.shape if dims is None else dims
        _lib.check(lib.trace_op_avgpool(_ptr(x), _ptr(y), int(N), int(HW), int(Cn), _stream()))
        return y

    @staticmethod
    def bias_act(x, bias, act, dims=None):
        """trace_op_bias_act, in place: x [rows, C] = act(x + bias); bias [C] or None; act 0 none, 1 SiLU, 2 sigmoid, 3 GELU (exact erf)"""
        lib = ops._stc(x, bias)
        rows, Cn = x.shape if dims is None else dims
        _lib.check(lib.trace_op_bias_act(_ptr(x), _ptr(bias), int(rows), int(Cn), int(act), _stream()))
        return x

    @staticmethod
    def scale_rows(x, gate, dims=None):
        """trace_op_scale_rows, in place: x [N, HW, C] *= gate [N, C]"""
        lib = ops._stc(x, gate)
        N, HW, Cn = x.shape if dims is None else dims
        _lib.check(lib.trace_op_scale_rows(_ptr(x), _ptr(gate), int(N), int(HW), int(Cn), _stream()))
        return x

    @staticmethod
    def im2col3d(x, out=None, dims=None):
        """trace_op_im2col3d: x [T, H, W, C] -> A [(T // 2 + 1) (H // 2 + 1) (W // 2 + 1), 8 C], the patches of Conv3d(kernel 2, stride 2, padding 1);
        `out`: a buffer of at least that many elements to store into"""
        T, H, W, Cn = x.shape if dims is None else dims
        rows = (T // 2 + 1) * (H // 2 + 1) * (W // 2 + 1)
        A = torch.empty((rows, 8 * Cn), dtype=x.dtype, device=x.device) if out is None else out
        lib = ops._stc(x, A)
        if dims is None and A.numel() < rows * 8 * Cn:
            raise ValueError("out: room for [To Ho Wo, 8 C]")
        _lib.check(lib.trace_op_im2col3d(_ptr(x), _ptr(A), int(T), int(H), int(W), int(Cn), _stream()))
        return A if out is None else A.view(-1)[:rows * 8 * Cn].view(rows, 8 * Cn)

    @staticmethod
    def permute_conv3d_w(w, out=None, dims=None):
        """trace_op_permute_conv3d_w: Conv3d weight w [Co, Ci, 2, 2, 2] -> [Co, 8 Ci] (im2col3d's column order)"""
        Co, Ci = w.shape[:2] if dims is None else dims
        o = torch.empty((Co, 8 * Ci), dtype=w.dtype, device=w.device) if out is None else out
        lib = ops._stc(w, o)
        _lib.check(lib.trace_op_permute_conv3d_w(_ptr(w), _ptr(o), int(Co), int(Ci), _stream()))
        return o

    # ---- the prefill's cache-write kernels (trace_hip.h: "the prefill's cache-write kernels, each alone") ----
    # Every array is a contiguous tensor whose numel() is the element count the library checks against and whose data_ptr() is the base the kernel gets:
    # an offset into a larger buffer is a slice of its flat view (buf.view(-1)[off:]).  Strides and offsets go through as given.
    @staticmethod
    def _flat(t, name, dtype=None):
        if t is None:
            return None
        if not t.is_contiguous() or (dtype is not None and t.dtype != dtype):
            raise ValueError(f"{name}: a contiguous tensor" + (f" of {dtype}" if dtype is not None else ""))
        return t

    @staticmethod
    def rope_kv(qkv, ld, kcache, slot_stride, kv_head_stride, R, nq, nkv, hd, cos_t, sin_t, slot0=0, pos0=0, seq_len=0, slot_arr=None, pos_arr=None,
                vcache=None, table_rows=None):
        """trace_op_rope_kv, in place on qkv / kcache / vcache.  cos_t, sin_t: fp32 [table_rows, hd / 2] (table_rows=None: the rows the tensors hold);
        slot_arr / pos_arr: int32 device tensors."""
        lib = _lib.load(ops.element)
        el = ops.dtype()
        for t, name in ((qkv, "qkv"), (kcache, "kcache"), (vcache, "vcache")):
            ops._flat(t, name, el)
        for t, name in ((cos_t, "cos_t"), (sin_t, "sin_t")):
            ops._flat(t, name, torch.float32)
        for t, name in ((slot_arr, "slot_arr"), (pos_arr, "pos_arr")):
            ops._flat(t, name, torch.int32)
        if cos_t.numel() != sin_t.numel() or (slot_arr is not None and pos_arr is not None and slot_arr.numel() != pos_arr.numel()):
            raise ValueError("cos_t / sin_t, slot_arr / pos_arr: equal sizes")
        rows = cos_t.numel() // max(hd // 2, 1) if table_rows is None else int(table_rows)
        if rows * (hd // 2) > cos_t.numel():
            raise ValueError("table_rows: more rows than the tables hold")
        arr = slot_arr if slot_arr is not None else pos_arr
        _lib.check(lib.trace_op_rope_kv(_ptr(qkv), qkv.numel(), int(ld), _ptr(kcache), kcache.numel(), _ptr(vcache), 0 if vcache is None else vcache.numel(),
                                        int(slot_stride), int(kv_head_stride), _ptr(slot_arr), _ptr(pos_arr), 0 if arr is None else arr.numel(), int(slot0),
                                        int(pos0), int(R), int(nq), int(nkv), int(hd), _ptr(cos_t), _ptr(sin_t), rows, int(seq_len), _stream()))

    @staticmethod
    def transpose_v(src, src_bs, src_hs, src_rs, dst, dst_bs, dst_hs, dst_rs, n, hd, heads, batch, perm=0, p0=0):
        """trace_op_transpose_v, in place on dst"""
        lib = _lib.load(ops.element)
        ops._flat(src, "src", ops.dtype())
        ops._flat(dst, "dst", ops.dtype())
        _lib.check(lib.trace_op_transpose_v(_ptr(src), src.numel(), int(src_bs), int(src_hs), int(src_rs), _ptr(dst), dst.numel(), int(dst_bs), int(dst_hs),
                                            int(dst_rs), int(n), int(hd), int(heads), int(batch), int(perm), int(p0), _stream()))

    @staticmethod
    def gather_rows(tabs, kind, row, out, L, H, tab_rows=None):
        """trace_op_gather_rows, in place on out.  tabs: six tensors [rows, H] or None; tab_rows=None: the rows each tensor holds; kind / row: int32 device
        tensors."""
        lib = _lib.load(ops.element)
        if len(tabs) != 6:
            raise ValueError("tabs: six tables (None = unused)")
        for t in tabs:
            ops._flat(t, "table", ops.dtype())
        ops._flat(out, "out", ops.dtype())
        ops._flat(kind, "kind", torch.int32)
        ops._flat(row, "row", torch.int32)
        counts = [0 if t is None else t.numel() // max(int(H), 1) for t in tabs] if tab_rows is None else [int(x) for x in tab_rows]
        if any(c * int(H) > (0 if t is None else t.numel()) for c, t in zip(counts, tabs)):
            raise ValueError("tab_rows: more rows than a table holds")
        ptrs = (C.c_void_p * 6)(*[None if t is None else t.data_ptr() for t in tabs])
        _lib.check(lib.trace_op_gather_rows(ptrs, (C.c_int64 * 6)(*counts), _ptr(kind), kind.numel(), _ptr(row), row.numel(), _ptr(out), out.numel(), int(L),
                                            int(H), _stream()))

    @staticmethod
    def slot_pool(feats, ln_w, ln_b, slots, cos_t, sin_t, eps):
        """trace_op_slot_pool: feats [T, n, D] — a view with unit channel stride, any frame / row strides that are multiples of 8 elements — ln_w / ln_b
        [D], slots [D, 8], cos_t / sin_t fp32 [n, D / 2] -> res [T, 8, D] (SpatialSlotPool before `readout`)."""
        lib = _lib.load(ops.element)
        if feats.dim() != 3 or feats.stride(2) != 1:
            raise ValueError("feats: [T, n, D] with unit channel stride")
        T, n, D = feats.shape
        cos_t, sin_t = cos_t.contiguous(), sin_t.contiguous()
        if tuple(slots.shape) != (D, 8) or tuple(cos_t.shape) != (n, D // 2) or tuple(sin_t.shape) != (n, D // 2) or cos_t.dtype != torch.float32 \
                or sin_t.dtype != torch.float32:
            raise ValueError("slots [D, 8]; cos_t / sin_t fp32 [n, D / 2]")
        nws = int(lib.trace_op_slot_pool_ws_floats(T, D))
        if nws < 0:
            raise _lib.TraceHipError(f"error {nws} in trace_op_slot_pool_ws_floats")
        ws = torch.empty(nws, dtype=torch.float32, device=feats.device)
        out = torch.empty((T, 8, D), dtype=feats.dtype, device=feats.device)
        _lib.check(lib.trace_op_slot_pool(_ptr(feats), feats.stride(0) if T > 1 else n * feats.stride(1), feats.stride(1), _ptr(ln_w.contiguous()),
                                          _ptr(ln_b.contiguous()), _ptr(slots.contiguous()), _ptr(cos_t), _ptr(sin_t), _ptr(out), T, n, D, float(eps),
                                          _ptr(ws), nws, _stream()))
        return out

    @staticmethod
    def patch_embed(frames, conv_w, cls, pos, pre_w, pre_b, P, eps, out=None):
        """trace_op_patch_embed: frames [T, 3, S, S] (the element type, or fp32), conv_w [D, 3 P P] (or [D, 3, P, P]), cls [D], pos [G G + 1, D],
        pre_w / pre_b [D] -> X [T, G G + 1, D] = pre_layrnorm(cat(CLS, conv(frames)) + pos).  `out`: a flat buffer of at least T (G G + 1) D elements to
        store into (a test's buffer with guard rows) instead of a fresh tensor.  TraceHipError (TRACE_ERR_ARG) for a geometry the fused kernel does not
        take."""
        lib = _lib.load(ops.element)
        dt = ops.dtype()
        if frames.dim() != 4 or frames.shape[1] != 3 or frames.shape[2] != frames.shape[3] or frames.dtype not in (dt, torch.float32):
            raise ValueError("frames: [T, 3, S, S] in the element type or fp32")
        frames = frames.contiguous()
        T, S = frames.shape[0], frames.shape[2]
        D = conv_w.shape[0]
        w = conv_w.reshape(D, -1).contiguous()
        G = S // max(P, 1)
        nws = int(lib.trace_op_patch_embed_ws_elems(P, D))
        taken = nws >= 0 and S % P == 0                                        # (else the op answers TRACE_ERR_ARG before it reads anything)
        if any(t.dtype != dt for t in (w, cls, pos, pre_w, pre_b)) or (taken and (w.shape[1] != 3 * P * P or tuple(pos.shape) != (G * G + 1, D)
                                                                                  or cls.numel() != D or pre_w.numel() != D or pre_b.numel() != D)):
            raise ValueError("conv_w [D, 3 P P], cls / pre_w / pre_b [D], pos [G G + 1, D], all in the element type")
        ws = torch.empty(max(nws, 8), dtype=dt, device=frames.device)          # (a refused geometry: the op itself answers TRACE_ERR_ARG)
        if out is None:
            out = torch.empty(T * (G * G + 1) * D, dtype=dt, device=frames.device)
        elif out.dim() != 1 or not out.is_contiguous() or out.dtype != dt or out.device != frames.device or out.numel() < T * (G * G + 1) * D:
            raise ValueError("out: a flat contiguous buffer of the element type with room for [T, G G + 1, D]")
        _lib.check(lib.trace_op_patch_embed(_ptr(frames), 1 if frames.dtype == torch.float32 else 0, _ptr(w), _ptr(cls.contiguous()),
                                            _ptr(pos.contiguous()), _ptr(pre_w.contiguous()), _ptr(pre_b.contiguous()), _ptr(out), T, S, P, D,
                                            float(eps), _ptr(ws), max(nws, 0), _stream()))
        return out[:T * (G * G + 1) * D].view(T, G * G + 1, D)

    @staticmethod
    def attention(q, k, v, causal, scale):
        """q [B, nq, heads, hd]; k, v [B, nkv, kv_heads, hd] -> [B, nq, heads, hd]"""
        lib = _lib.load(ops.element)
        Bn, nq, heads, hd = q.shape
        nkv, kvh = k.shape[1], k.shape[2]
        pad = (nkv + 63) // 64 * 64
        vt = torch.empty((Bn * kvh * hd * pad,), dtype=ops.dtype(), device=q.device)
        o = torch.empty_like(q)
        _lib.check(lib.trace_op_attention(_ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(vt), Bn, heads, kvh, nq, nkv, hd,
                                          1 if causal else 0, scale, _stream()))
        return o

    @staticmethod
    def tile_pack(W):
        """row-major [N, K] -> the decode GEMV tile layout (same shape/bytes, permuted)"""
        lib = _lib.load(ops.element)
        out = torch.empty_like(W)
        _lib.check(lib.trace_op_tile_pack(_ptr(W), _ptr(out), W.shape[0], W.shape[1], _stream()))
        return out

    @staticmethod
    def skinny_gemm(X, W, R=None, epilogue=EPI_NONE, tiled=False, want_partial=True):
        """decode GEMV; `tiled`: W was passed through tile_pack.  EPI_PARTIAL returns the fp32 partial rows [KS, sk_rows, N]."""
        lib = _lib.load(ops.element)
        Bn, K = X.shape
        N = W.shape[0]
        if epilogue == EPI_PARTIAL:
            ks = lib.trace_op_skinny_ks(N, K, epilogue, Bn)
            out = torch.zeros((ks, lib.trace_op_sk_rows(), N), dtype=torch.float32, device=X.device) if want_partial else None
        else:
            No = N // 2 if epilogue == EPI_SWIGLU else N
            out = torch.empty((Bn, No), dtype=ops.dtype(), device=X.device)
        _lib.check(lib.trace_op_skinny_gemm(_ptr(X), _ptr(W), _ptr(out), _ptr(R), Bn, N, K, epilogue, int(tiled), _stream()))
        return out

    @staticmethod
    def gemm_partial(X, W, tiled: int = 0):
        """decode batches above 64 rows: X [M <= 128, K] . W [N, K]^T as fp32 k-chunk partial rows [ks, sk_rows, N] (split-K MFMA GEMM);
        tiled: W went through tile_pack (1; 5 = + the 4-stage K-tile ring)"""
        lib = _lib.load(ops.element)
        M, K = X.shape
        N = W.shape[0]
        out = torch.zeros((lib.trace_op_gemm_partial_ks(N, K), lib.trace_op_sk_rows(), N), dtype=torch.float32, device=X.device)
        _lib.check(lib.trace_op_gemm_partial(_ptr(X), _ptr(W), _ptr(out), M, N, K, int(tiled), _stream()))
        return out

    @staticmethod
    def gemm_swiglu_tiled(X, Wt, ring: bool = True):
        """gate|up of a wide decode step: X [M <= 128, K], Wt = tile_pack(16-row interleaved gate|up [N, K]) -> [M, N/2] bf16"""
        lib = _lib.load(ops.element)
        M, K = X.shape
        N = Wt.shape[0]
        out = torch.empty((M, N // 2), dtype=ops.dtype(), device=X.device)
        _lib.check(lib.trace_op_gemm_swiglu_tiled(_ptr(X), _ptr(Wt), _ptr(out), M, N, K, int(ring), _stream()))
        return out

    @staticmethod
    def skinny_fused_norm(part_in, R, w, eps, W, KS=None):
        """(xout, out-partials): xout = bf16(sum_k part_in[k, :B]) + R; partial rows [ks, sk_rows, N] of RMSNorm(xout; w) . W^T  (B <= 4).
        KS: chunks of part_in to read (default: all the tensor holds)"""
        lib = _lib.load(ops.element)
        Bn, K = R.shape
        N = W.shape[0]
        ks_in = 0 if part_in is None else (part_in.shape[0] if KS is None else int(KS))
        xout = torch.empty_like(R)
        out = torch.zeros((lib.trace_op_skinny_ks(N, K, EPI_PARTIAL, Bn), lib.trace_op_sk_rows(), N), dtype=torch.float32, device=R.device)
        _lib.check(lib.trace_op_skinny_fused_norm(_ptr(part_in), ks_in, _ptr(R), _ptr(xout), _ptr(w), eps, _ptr(W), _ptr(out), Bn, N, K, _stream()))
        return xout, out

    @staticmethod
    def skinny_ks(N, K, epilogue, B):
        return _lib.load(ops.element).trace_op_skinny_ks(N, K, epilogue, B)

    @staticmethod
    def skinny_plan(kind, N, K, epilogue, B) -> dict:
        """trace_op_skinny_plan: the workgroup partition of one decode GEMV (kind 0 bf16, 1 W8A8, 2 W8A16) and its partial-row floats"""
        out = (C.c_int64 * 11)()
        _lib.check(_lib.load(ops.element).trace_op_skinny_plan(kind, N, K, epilogue, B, out))
        return dict(zip(("KS", "chunk_units", "T", "WPT", "ntiles", "grid", "threads", "NT", "NB", "lds_bytes", "partial_floats"), out))

    @staticmethod
    def decode_route(B, fp8_scheme, H, I, QKV) -> dict:
        """trace_op_decode_route: what a decode step of B sequences does under the current tuning values ('step' = get_profile()[8])"""
        out = (C.c_int32 * 8)()
        _lib.check(_lib.load(ops.element).trace_op_decode_route(B, fp8_scheme, H, I, QKV, out))
        return dict(zip(("step", "kind", "qkv_finish", "ks_q", "ks_o", "ks_g", "ks_d", "nsplit"), out))

    @staticmethod
    def swiglu_combine(part, Bn):
        lib = _lib.load(ops.element)
        N2 = part.shape[2]
        out = torch.empty((Bn, N2 // 2), dtype=ops.dtype(), device=part.device)
        _lib.check(lib.trace_op_swiglu_combine(_ptr(part), part.shape[0], N2, _ptr(out), Bn, _stream()))
        return out

    @staticmethod
    def add_rmsnorm(part, R, w, eps):
        """(x, y): x = bf16(sum_ks part[ks, b]) + R[b]; y = RMSNorm(x) * w"""
        lib = _lib.load(ops.element)
        Bn, N = R.shape
        x, y = torch.empty_like(R), torch.empty_like(R)
        _lib.check(lib.trace_op_add_rmsnorm(_ptr(part), part.shape[0], _ptr(R), _ptr(x), _ptr(w), _ptr(y), Bn, N, eps, _stream()))
        return x, y

    @staticmethod
    def add_rmsnorm_ex(part, R, w, eps, KS=None, xout=None, y=None, fp8=False):
        """trace_op_add_rmsnorm_ex.  part fp32 [>= KS, sk_rows, N] (KS=None: every chunk of the tensor); R, `xout`, `y` [B, N], strided views allowed
        (unit column stride; a view's row stride is what the kernel gets); xout=None / y=None: fresh contiguous tensors; xout may be R (in place, the
        engine's form).  fp8: also the e4m3 bytes and row scales of y.  Returns (xout, y) or (xout, y, y8, sy)."""
        lib = _lib.load(ops.element)
        ops._rows2d(R, "R")
        Bn, N = R.shape
        x = torch.empty((Bn, N), dtype=R.dtype, device=R.device) if xout is None else ops._rows2d(xout, "xout")
        yy = torch.empty((Bn, N), dtype=R.dtype, device=R.device) if y is None else ops._rows2d(y, "y")
        if tuple(x.shape) != (Bn, N) or tuple(yy.shape) != (Bn, N):
            raise ValueError("xout / y: the shape of R")
        if part.dim() != 3 or part.dtype != torch.float32 or not part.is_contiguous() or part.shape[1] != lib.trace_op_sk_rows() or part.shape[2] != N:
            raise ValueError("part: contiguous fp32 [chunks, sk_rows, N]")
        ks = part.shape[0] if KS is None else int(KS)
        if ks > part.shape[0]:
            raise ValueError("KS: more chunks than the tensor holds")
        y8 = torch.empty((Bn, N), dtype=torch.uint8, device=R.device) if fp8 else None
        sy = torch.empty((Bn,), dtype=torch.float32, device=R.device) if fp8 else None
        _lib.check(lib.trace_op_add_rmsnorm_ex(_ptr(part), ks, _ptr(R), R.stride(0), _ptr(x), x.stride(0), _ptr(w), _ptr(yy), yy.stride(0), _ptr(y8), _ptr(sy),
                                               Bn, N, float(eps), _stream()))
        return (x, yy, y8, sy) if fp8 else (x, yy)

    @staticmethod
    def skinny_fused_swiglu(part_gu, W, Bn, KS=None):
        """trace_op_skinny_fused_swiglu: part_gu fp32 [>= KS, sk_rows, 2 K] (16-row interleaved gate|up partial rows), W [N, K] row-major -> the fp32
        partial rows [ks, sk_rows, N] of el(silu(sum gate) * sum up) . W^T  (Bn <= 4)"""
        lib = _lib.load(ops.element)
        N, K = W.shape
        if part_gu.dim() != 3 or part_gu.dtype != torch.float32 or not part_gu.is_contiguous() or part_gu.shape[1] != lib.trace_op_sk_rows() \
                or part_gu.shape[2] != 2 * K:
            raise ValueError("part_gu: contiguous fp32 [chunks, sk_rows, 2 K]")
        ks_gu = part_gu.shape[0] if KS is None else int(KS)
        if ks_gu > part_gu.shape[0]:
            raise ValueError("KS: more chunks than the tensor holds")
        ks = lib.trace_op_skinny_ks(N, K, EPI_PARTIAL, Bn) if (1 <= Bn <= 64 and N >= 16 and N % 16 == 0 and K >= 64 and K % 64 == 0) else 1
        out = torch.zeros((ks, lib.trace_op_sk_rows(), N), dtype=torch.float32, device=W.device)
        _lib.check(lib.trace_op_skinny_fused_swiglu(_ptr(part_gu), ks_gu, _ptr(W.contiguous()), _ptr(out), Bn, N, K, _stream()))
        return out

    @staticmethod
    def attn_decode(q, kcache, vcache, pos, nsplit, scale, vtcache=None):
        """q [B, nq*128]; caches [B, nkv, max_ctx, 128]; pos int32 [B] (device).  The kernel reads V transposed
        ([B, nkv, 128, max_ctx], the engine's cache layout): built here unless `vtcache` is passed."""
        lib = _lib.load(ops.element)
        if vtcache is None:
            vtcache = vcache.transpose(2, 3).contiguous()
        vcache = vtcache
        Bn = q.shape[0]
        nkv, max_ctx = kcache.shape[1], kcache.shape[2]
        nq = q.shape[1] // 128
        ws = torch.zeros((Bn * nq * nsplit * 130,), dtype=torch.float32, device=q.device)
        o = torch.empty_like(q)
        _lib.check(lib.trace_op_attn_decode(_ptr(q), _ptr(kcache), _ptr(vcache), _ptr(pos), _ptr(o), _ptr(ws), Bn, nq, nkv,
                                            max_ctx, nsplit, scale, _stream()))
        return o

    @staticmethod
    def attn_decode_shared(q, kcache, vtcache, pos, nsplit, scale, shared_slot, shared_rows):
        """attn_decode over caches of S >= B slots (kcache [S, nkv, max_ctx, 128], vtcache [S, nkv, 128, max_ctx]; row b in slot b) with positions
        below shared_rows of every row read from slot shared_slot (trace_op_attn_decode_shared)."""
        lib = _lib.load(ops.element)
        Bn = q.shape[0]
        S, nkv, max_ctx = kcache.shape[0], kcache.shape[1], kcache.shape[2]
        nq = q.shape[1] // 128
        ws = torch.zeros((Bn * nq * nsplit * 130,), dtype=torch.float32, device=q.device)
        o = torch.empty_like(q)
        _lib.check(lib.trace_op_attn_decode_shared(_ptr(q), _ptr(kcache), _ptr(vtcache), _ptr(pos), _ptr(o), _ptr(ws), Bn, nq, nkv, S, max_ctx, nsplit,
                                                   scale, int(shared_slot), int(shared_rows), _stream()))
        return o

    @staticmethod
    def sk_rows() -> int:
        return _lib.load(ops.element).trace_op_sk_rows()

    @staticmethod
    def qkv_finish(part, kcache, vtcache, slots, pos, cos_t, sin_t, nq):
        """part fp32 [ks, sk_rows, (nq + 2 nkv) * 128] -> roped q rows [B, nq * 128]; the K row and the V^T column of row b are stored IN PLACE at
        pos[b] of slot slots[b] of kcache [S, nkv, max_ctx, 128] / vtcache [S, nkv, 128, max_ctx].  slots, pos int32 [B] (device); cos_t, sin_t
        fp32 [max_ctx, 64]."""
        lib = _lib.load(ops.element)
        S, nkv, max_ctx = kcache.shape[0], kcache.shape[1], kcache.shape[2]
        Bn = pos.shape[0]
        qkv = torch.zeros((Bn, (nq + 2 * nkv) * 128), dtype=ops.dtype(), device=part.device)
        _lib.check(lib.trace_op_qkv_finish(_ptr(part), part.shape[0], _ptr(qkv), _ptr(kcache), _ptr(vtcache), _ptr(slots), _ptr(pos), _ptr(cos_t),
                                           _ptr(sin_t), Bn, nq, nkv, S, max_ctx, _stream()))
        return qkv[:, :nq * 128].contiguous()

    @staticmethod
    def attn_decode_fused(part, kcache, vtcache, slots, pos, cos_t, sin_t, nq, nsplit, scale):
        """The decode attention with its fused prologue: qkv_finish's inputs (caches appended IN PLACE) -> attention output [B, nq * 128]."""
        lib = _lib.load(ops.element)
        S, nkv, max_ctx = kcache.shape[0], kcache.shape[1], kcache.shape[2]
        Bn = pos.shape[0]
        ws = torch.zeros((Bn * nq * nsplit * 130,), dtype=torch.float32, device=part.device)
        o = torch.empty((Bn, nq * 128), dtype=ops.dtype(), device=part.device)
        _lib.check(lib.trace_op_attn_decode_fused(_ptr(part), part.shape[0], _ptr(kcache), _ptr(vtcache), _ptr(slots), _ptr(pos), _ptr(cos_t),
                                                  _ptr(sin_t), _ptr(o), _ptr(ws), Bn, nq, nkv, S, max_ctx, nsplit, scale, _stream()))
        return o

    # ---- e4m3 KV cache (trace_amd/kv8.py states the format and the four arrays) ----
    @staticmethod
    def attn_decode_kv8(q, k8, v8, ks, vs, pos, nsplit, scale):
        """q [B, nq*128] rotated; k8 uint8 [B, nkv, max_ctx, 128], v8 uint8 [B, nkv, max_ctx/32, 128, 32], ks / vs fp32 [B, nkv, max_ctx] (row b in
        slot b); pos int32 [B] (device) -> [B, nq*128]"""
        lib = _lib.load(ops.element)
        Bn, nq = q.shape[0], q.shape[1] // 128
        nkv, max_ctx = k8.shape[1], k8.shape[2]
        ws = torch.zeros((Bn * nq * nsplit * 130,), dtype=torch.float32, device=q.device)
        o = torch.empty_like(q)
        _lib.check(lib.trace_op_attn_decode_kv8(_ptr(q), _ptr(k8), _ptr(v8), _ptr(ks), _ptr(vs), _ptr(pos), _ptr(o), _ptr(ws), Bn, nq, nkv, max_ctx,
                                                nsplit, scale, _stream()))
        return o

    @staticmethod
    def qkv_finish_kv8(part, k8, v8, ks, vs, slots, pos, cos_t, sin_t, nq):
        """ops.qkv_finish for kv8 arrays [S, ...]: roped q rows [B, nq * 128]; the new k row / v column quantised and stored IN PLACE with their scales"""
        lib = _lib.load(ops.element)
        S, nkv, max_ctx = k8.shape[0], k8.shape[1], k8.shape[2]
        Bn = pos.shape[0]
        qkv = torch.zeros((Bn, (nq + 2 * nkv) * 128), dtype=ops.dtype(), device=part.device)
        _lib.check(lib.trace_op_qkv_finish_kv8(_ptr(part), part.shape[0], _ptr(qkv), _ptr(k8), _ptr(v8), _ptr(ks), _ptr(vs), _ptr(slots), _ptr(pos),
                                               _ptr(cos_t), _ptr(sin_t), Bn, nq, nkv, S, max_ctx, _stream()))
        return qkv[:, :nq * 128].contiguous()

    @staticmethod
    def kv8_pack(k_rows, v_rows, k8, v8, ks, vs, slots, pos0):
        """k_rows (roped) / v_rows [B, nkv, R, 128] in the element type -> positions pos0 .. pos0 + R - 1 of slot slots[b] of the kv8 arrays, IN PLACE"""
        lib = _lib.load(ops.element)
        Bn, nkv, R = k_rows.shape[0], k_rows.shape[1], k_rows.shape[2]
        _lib.check(lib.trace_op_kv8_pack(_ptr(k_rows.contiguous()), _ptr(v_rows.contiguous()), _ptr(k8), _ptr(v8), _ptr(ks), _ptr(vs), _ptr(slots),
                                         pos0, R, Bn, nkv, k8.shape[0], k8.shape[2], _stream()))

    @staticmethod
    def kv8_unpack(k8, v8, ks, vs, slots, R, k_out=None, vt_out=None):
        """positions 0 .. R - 1 of slot slots[b] -> row b of (k [B, nkv, max_ctx, 128], V^T [B, nkv, 128, max_ctx]) in the element type; positions from R
        on keep what k_out / vt_out held (zeros when they are made here)"""
        lib = _lib.load(ops.element)
        Bn, nkv, max_ctx = slots.shape[0], k8.shape[1], k8.shape[2]
        if k_out is None:
            k_out = torch.zeros((Bn, nkv, max_ctx, 128), dtype=ops.dtype(), device=k8.device)
        if vt_out is None:
            vt_out = torch.zeros((Bn, nkv, 128, max_ctx), dtype=ops.dtype(), device=k8.device)
        _lib.check(lib.trace_op_kv8_unpack(_ptr(k8), _ptr(v8), _ptr(ks), _ptr(vs), _ptr(slots), _ptr(k_out), _ptr(vt_out), R, Bn, nkv, k8.shape[0],
                                           max_ctx, _stream()))
        return k_out, vt_out

    # ---- w4 path pieces (the format: trace_amd/w4.py) ----
    @staticmethod
    def skinny_w4_plan(N, K, B) -> dict:
        """trace_op_skinny_w4_plan: skinny_plan for the w4 decode GEMV (units of 256 k)"""
        out = (C.c_int64 * 11)()
        _lib.check(_lib.load(ops.element).trace_op_skinny_w4_plan(N, K, B, out))
        return dict(zip(("KS", "chunk_units", "T", "WPT", "ntiles", "grid", "threads", "NT", "NB", "lds_bytes", "partial_floats"), out))

    @staticmethod
    def decode_route_w4(B, H, I, QKV) -> dict:
        """trace_op_decode_route_w4: decode_route for a context on w4 weights"""
        out = (C.c_int32 * 8)()
        _lib.check(_lib.load(ops.element).trace_op_decode_route_w4(B, H, I, QKV, out))
        return dict(zip(("step", "kind", "qkv_finish", "ks_q", "ks_o", "ks_g", "ks_d", "nsplit"), out))

    @staticmethod
    def quant_rows_w4(W):
        """W bf16 [N, K] -> (uint8 codes [N, K / 2], uint8 exponent bytes [N, K / 32]) in the logical order"""
        lib = _lib.load(ops.element)
        N, K = W.shape
        codes = torch.empty((N, K // 2), dtype=torch.uint8, device=W.device)
        exps = torch.empty((N, K // 32), dtype=torch.uint8, device=W.device)
        _lib.check(lib.trace_op_quant_rows_w4(_ptr(W), _ptr(codes), _ptr(exps), N, K, _stream()))
        return codes, exps

    @staticmethod
    def tile_pack_w4(codes, exps):
        """logical codes / exponents -> the decode tile copies (flat uint8 [N K / 2], [N K / 32])"""
        lib = _lib.load(ops.element)
        N, K = codes.shape[0], codes.shape[1] * 2
        tc, te = torch.empty(N * K // 2, dtype=torch.uint8, device=codes.device), torch.empty(N * K // 32, dtype=torch.uint8, device=codes.device)
        _lib.check(lib.trace_op_tile_pack_w4(_ptr(codes), _ptr(exps), _ptr(tc), _ptr(te), N, K, _stream()))
        return tc, te

    @staticmethod
    def dequant_w4(tcodes, texps, N, K):
        """the tile copies -> W~ bf16 [N, K], exact"""
        lib = _lib.load(ops.element)
        out = torch.empty((N, K), dtype=torch.bfloat16, device=tcodes.device)
        _lib.check(lib.trace_op_dequant_w4(_ptr(tcodes), _ptr(texps), _ptr(out), N, K, _stream()))
        return out

    @staticmethod
    def skinny_w4(X, tcodes, texps, N, out=None):
        """the w4 decode GEMV: X bf16 [B, K] . W~^T as fp32 k-chunk partial rows [KS, sk_rows, N], written into `out` if one is given (rows >= B of a
        chunk are not written); the product is out.sum(0)[:B]"""
        lib = _lib.load(ops.element)
        Bn, K = X.shape
        if out is None:
            out = torch.zeros((ops.skinny_w4_plan(N, K, Bn)["KS"], lib.trace_op_sk_rows(), N), dtype=torch.float32, device=X.device)
        _lib.check(lib.trace_op_skinny_w4(_ptr(X), _ptr(tcodes), _ptr(texps), _ptr(out), Bn, N, K, _stream()))
        return out

    # ---- fp8 (e4m3) path pieces ----
    @staticmethod
    def quant_rows_fp8(X):
        """X bf16 [rows, K] -> (uint8 e4m3 bytes [rows, K], fp32 scale [rows])"""
        lib = _lib.load(ops.element)
        q = torch.empty(X.shape, dtype=torch.uint8, device=X.device)
        sx = torch.empty((X.shape[0],), dtype=torch.float32, device=X.device)
        _lib.check(lib.trace_op_quant_rows_fp8(_ptr(X), _ptr(q), _ptr(sx), X.shape[0], X.shape[1], _stream()))
        return q, sx

    @staticmethod
    def gemm_fp8(A8, sa, W8, sw, R=None, epilogue=EPI_NONE):
        lib = _lib.load(ops.element)
        M, K = A8.shape
        N = W8.shape[0]
        No = N // 2 if epilogue == EPI_SWIGLU else N
        Cc = torch.empty((M, No), dtype=ops.dtype(), device=A8.device)
        _lib.check(lib.trace_op_gemm_fp8(_ptr(A8), _ptr(sa), _ptr(W8), _ptr(sw), _ptr(Cc), _ptr(R), M, N, K, epilogue, _stream()))
        return Cc

    @staticmethod
    def skinny_w8(X, W8, sw):
        """weight-only decode GEMV: X bf16 [B, K], W8 uint8 e4m3 [N, K] + row scales -> fp32 [B, N]"""
        lib = _lib.load(ops.element)
        Bn, K = X.shape
        N = W8.shape[0]
        out = torch.empty((Bn, N), dtype=torch.float32, device=X.device)
        _lib.check(lib.trace_op_skinny_w8(_ptr(X), _ptr(W8), _ptr(sw), _ptr(out), Bn, N, K, _stream()))
        return out

    @staticmethod
    def skinny_fp8(X8, sx, W8, sw):
        lib = _lib.load(ops.element)
        Bn, K = X8.shape
        N = W8.shape[0]
        out = torch.empty((Bn, N), dtype=torch.float32, device=X8.device)
        _lib.check(lib.trace_op_skinny_fp8(_ptr(X8), _ptr(sx), _ptr(W8), _ptr(sw), _ptr(out), Bn, N, K, _stream()))
        return out
