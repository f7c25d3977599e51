"""Host-side `TraceMistralForCausalLM` with the reference's call surface (trace/model/language_model/
trace_mistral.py): `.generate(inputs, images_or_videos=, modal_list=, video_timestamps=, heads=, max_new_tokens=,
do_sample=, ...) -> LongTensor[B, n_new]`, `.forward(...)` -> object with `.logits`, `.config`, `.get_model()`,
`.get_vision_tower()`, `.to()`, `.eval()`.  Everything between the frame tensor and the token ids runs in the HIP
engine (trace_amd/engine.py -> libtrace_hip.so); this class only adapts arguments."""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import scoring
from ..config import TraceConfig
from ..constants import MMODAL_TOKEN_INDEX, NUM_FRAMES
from ..prefix import split_questions
from ..sampling import Constraints, LogitsParams, SamplingParams, check_constraints, check_sampling
from .encoders import NumberTokenizer, ScoreTower, TimeTower


class _VisionTower:
    """Attribute holder standing in for CLIPVisionTower (clip_encoder.py): drivers read `.image_processor`."""

    def __init__(self, cfg: TraceConfig, image_processor):
        self.config = SimpleNamespace(hidden_size=cfg.vision_hidden_size, image_size=cfg.vision_image_size,
                                      patch_size=cfg.vision_patch_size)
        self.image_processor = image_processor
        self.is_loaded = True
        self.hidden_size = cfg.vision_hidden_size
        self.num_patches = cfg.vision_patches

    def load_model(self):
        return None

    def to(self, *a, **k):
        return self


class _MetaModel:
    """`model.get_model()`: exposes the tokenizers/towers the drivers touch (trace_arch.py:31-40)."""

    def __init__(self, cfg: TraceConfig, vision_tower: _VisionTower):
        self.time_tokenizer = NumberTokenizer()
        self.score_tokenizer = NumberTokenizer()
        self.time_tower = TimeTower(self.time_tokenizer)
        self.score_tower = ScoreTower(self.score_tokenizer)
        self.vision_tower = vision_tower

    def get_vision_tower(self):
        return self.vision_tower

    def get_time_tower(self):
        return self.time_tower

    def get_score_tower(self):
        return self.score_tower


class TraceMistralForCausalLM:
    def __init__(self, config: TraceConfig, engine, image_processor=None):
        self.config = config
        self.engine = engine
        self.vocab_size = config.vocab_size
        self.time_vocab_size = config.time_vocab_size
        self.score_vocab_size = config.score_vocab_size
        # trace_mistral.py:86-88
        self.swap_tokens = {config.vocab_size: 1, config.vocab_size + 1: 2,
                            config.vocab_size + config.time_vocab_size + 1: 0}
        self.model = _MetaModel(config, _VisionTower(config, image_processor))
        self.device = engine.device
        self.dtype = engine.dtype
        # HF GenerationConfig defaults; builder.load_pretrained_model overrides them from the checkpoint's generation_config.json
        self.generation_config = SimpleNamespace(do_sample=False, temperature=1.0, top_k=50, top_p=1.0, repetition_penalty=1.0, no_repeat_ngram_size=0,
                                                 min_new_tokens=0)
        self._prefix_cache = False

    # ---- prompt-prefix reuse across generate() calls ----
    def enable_prefix_cache(self, on: bool = True):
        """One video, several questions (the reference's drivers call generate once per question with the same frame tensor and a prompt that
        is identical through `<video>`, trace/eval/videomme/evaluate.py:349-386): with the cache on, generate() prefills a prompt in two
        passes — the rows through `<video>`, then the rows after it — and a B = 1 call whose frame tensor (the same object, not edited in
        place since), timestamps, modal and ids through `<video>` equal the previous call's skips the tower, the slot pool and the first pass:
        the rows are still in KV slot 0.  A B > 1 call whose rows all name one tensor object encodes and prefills the shared rows once
        (TraceEngine.generate_questions).  Results are bit-identical to the cache being off.  Off by default: an enabled cache keeps a
        reference to the caller's frame tensor after generate() returns; enable_prefix_cache(False) drops it."""
        self._prefix_cache = bool(on)
        self.engine._drop_prefix()
        return self

    @property
    def prefix_cache_enabled(self) -> bool:
        return self._prefix_cache

    @staticmethod
    def _ts_key(ts):
        """one tuple of stamps per frame"""
        return tuple(tuple(float(v) for v in (t if hasattr(t, "__iter__") else (t,))) for t in ts)

    def _prefix_lookup(self, raw, timestamps, modal, prefix):
        """(key, hit, rows): the prefix-cache key of one video's rows through `<video>` (the caller's tensor object and its version, the stamps, the
        modal, the ids), whether KV slot 0 still holds the rows of exactly that key, and how many rows it holds then (None on a miss).  The one
        place the key is made and compared: generate() and score() both ask here."""
        key = (raw, raw._version, self._ts_key(timestamps), modal, tuple(prefix))
        ent = self.engine.prefix_entry()
        hit = ent is not None and ent[0][0] is key[0] and ent[0][1:] == key[1:]
        return key, hit, (ent[1] if hit else None)

    def _generate_prefix_cached(self, raw, vids, modals, timestamps, id_lists, heads, max_new_tokens, eos, sampling, logprobs=False, **lg):
        """generate()'s main path with the cache on; None = this call is not of the cacheable shape (today's path runs)."""
        eng, B = self.engine, len(vids)
        try:
            prefix, suffixes = split_questions(id_lists)
        except ValueError:
            return None
        if any(len(x) == 0 for x in suffixes):
            return None
        ts_of = self._ts_key
        ts_key = ts_of(timestamps[0])
        if B > 1:
            if any(r is not raw[0] for r in raw[1:]) or any(m != modals[0] for m in modals[1:]) or any(ts_of(t) != ts_key for t in timestamps[1:]):
                return None
            if B > eng.decode_batch_max:
                return None
        key, hit, P = self._prefix_lookup(raw[0], timestamps[0], modals[0], prefix)
        if B > 1:
            return eng.generate_questions(vids[0], timestamps[0], id_lists, heads, max_new_tokens, eos=eos, sampling=sampling, prefix_key=key,
                                          logprobs=logprobs, **lg)
        if not hit:
            eng.encode_video(vids[0], timestamps[0])
            P = eng.splice(prefix)
            eng.prefill(0, P)
            eng.set_prefix_entry(key, P)
        eng.embed_rows(suffixes[0])
        eng.prefill_append(0, P, None, L=len(suffixes[0]))
        return eng.decode([0], heads, max_new_tokens, eos, sampling=sampling, logprobs=logprobs, **lg)

    # ---- nn.Module-like conveniences the drivers call ----
    def get_model(self):
        return self.model

    def get_vision_tower(self):
        return self.model.get_vision_tower()

    def to(self, *a, **k):
        return self

    def cuda(self, *a, **k):
        return self

    def half(self):
        return self

    def eval(self):
        return self

    def resize_token_embeddings(self, n):
        if n != self.config.vocab_size:
            raise NotImplementedError("the engine's embedding table is fixed at load time")

    # ---- generate (trace_mistral.py:268-314) ----
    @torch.no_grad()
    def generate(self, inputs=None, images_or_videos=None, times=None, scores=None, video_timestamps=None,
                 modal_list=None, heads=None, max_new_tokens: int = 128, do_sample: Optional[bool] = None,
                 temperature: Optional[float] = None, top_k: Optional[int] = None, top_p: Optional[float] = None, generation_config=None,
                 eos_token_id=None, pad_token_id: Optional[int] = None, stopping_criteria=None,
                 use_cache: bool = True, attention_mask=None, position_ids=None, output_logprobs: bool = False, retire_finished: bool = False,
                 **kwargs):
        """retire_finished=True: rows that have ended (EOS, a stop sequence) leave the running decode batch at chunk boundaries, so a batch of short
        and long answers stops paying for the short ones (TraceEngine.decode); the returned tensor has the same shape and rows.  Identical ids where
        the logits do not depend on rounding; on real weights a row that decodes on in a smaller batch sees that batch size's rounding
        (INTEGRATION.md 2a).  ValueError with stopping_criteria= and on the legacy STC path (both run the host loop).
        do_sample / temperature / top_k / top_p: explicit values, else `generation_config`'s, else this model's defaults (HF's: greedy,
        1.0, 50, 1.0, or the checkpoint's generation_config.json).  repetition_penalty / no_repeat_ngram_size / min_new_tokens: the same
        precedence; HF's processors in HF's order on the device, inside the decode step (trace_amd/csrc/logits.h).  Their history is the ids a row
        has generated so far, never the prompt (the reference hands HF inputs_embeds), as global vocabulary ids: a time or score digit emitted
        earlier counts in a later span too.  Log-probabilities keep describing the raw, unprocessed distribution.
        eos_token_id: an int or a list (HF's); the first id is the engine's eos, the others end a row the same way as stop sequences of one id.
        bad_words_ids / suppress_tokens / begin_suppress_tokens (HF's NoBadWords / SuppressTokens / SuppressTokensAtBegin processors) and
        stop_sequences (lists of global ids: a row ends once its generated ids end in one, the ids stay in the output): the same precedence, on
        the device inside the decode step (trace_amd/csrc/constrain.h) - no host loop.  stopping_criteria= still runs the host loop;
        mm_utils.stop_sequences_from_keywords(criterion) gives a KeywordsStoppingCriteria's ids for stop_sequences=.  Sampling follows HF's warpers (temperature -> top_k -> top_p ->
        min_p -> typical_p -> epsilon_cutoff -> eta_cutoff -> multinomial; the last four as keyword arguments with the same precedence, off by
        default) on the device (trace_amd/csrc/sample.h); the 64-bit seed is drawn from torch's default generator, so torch.manual_seed
        makes a call reproducible.  temperature == 0 or do_sample=False: greedy.
        output_logprobs=True: instead of the id tensor, an object with `.sequences` (exactly that tensor), `.logprobs` (float32 [B, n], zero
        padded: the log-probability of every emitted token under the model's own, unwarped distribution of the row's active head, computed
        on the device inside the decode step; a row's sum is its score) and `.heads` (the final heads)."""
        if "inputs_embeds" in kwargs:
            raise NotImplementedError("`inputs_embeds` is not supported")          # trace_mistral.py:282-283
        lgp = self._logits_params(kwargs.pop("repetition_penalty", None), kwargs.pop("no_repeat_ngram_size", None), kwargs.pop("min_new_tokens", None),
                                  generation_config)
        sampling = self._sampling_params(do_sample, temperature, top_k, top_p, _ProcessorsOff(generation_config, self.generation_config), kwargs)
        eos, cons = self._eos_and_constraints(eos_token_id, kwargs, generation_config)
        lg = {} if lgp is None else {"logits": lgp}              # handed on only when armed
        if cons is not None:
            lg["constraints"] = cons
        if retire_finished:
            lg["retire_finished"] = True                        # handed on only when on
        if images_or_videos is None:
            raise NotImplementedError("text-only generation is outside the accelerated path")
        cfg, eng = self.config, self.engine
        eng.host_mode(False)                    # a previous forward() leaves the engine armed for its decode form
        self._live_kv = None
        ids = inputs if isinstance(inputs, torch.Tensor) else torch.tensor(inputs)
        if ids.dim() == 1:
            ids = ids.unsqueeze(0)
        B = ids.shape[0]
        if len(images_or_videos) != B:
            raise ValueError("one video per prompt row")
        if heads is None:
            heads = [0] * B
        assert len(heads) == B                                                    # trace_mistral.py:245
        legacy_stc = video_timestamps is None and cfg.mm_projector_type == "stc_connector"
        if video_timestamps is None and not legacy_stc:
            raise ValueError("video_timestamps is required on the TRACE path (time tokens per frame)")
        modals = list(modal_list or ["video"] * B)
        vids = [self._as_frames(x, modal) for x, modal in zip(images_or_videos, modals)]
        id_lists = [row.tolist() for row in ids]
        if B > eng.max_batch:
            raise ValueError(f"batch {B} exceeds the engine's max_batch {eng.max_batch}")
        if retire_finished and (legacy_stc or stopping_criteria):
            raise ValueError("retire_finished=True needs the device decode loop: not with stopping_criteria= or on the legacy STC path")
        if legacy_stc:
            # legacy trace.infer() flow (trace/__init__.py:23-75): STC connector, no time tokens, text head only
            for b in range(B):
                eng.vit_forward(vids[b])
                eng.stc_connector(None, vids[b].shape[0])
                eng.prefill(b, eng.splice(id_lists[b]))
            out, new_heads, *lps = eng.decode(list(range(B)), [0] * B, max_new_tokens, eos, sampling=sampling, logprobs=output_logprobs, **lg)
        elif not stopping_criteria:
            res = None
            if self._prefix_cache and all(isinstance(x, torch.Tensor) for x in images_or_videos):
                res = self._generate_prefix_cached(list(images_or_videos), vids, modals, video_timestamps, id_lists, list(heads), max_new_tokens, eos, sampling,
                                                   output_logprobs, **lg)
            out, new_heads, *lps = res if res is not None else eng.generate(vids, video_timestamps, id_lists, list(heads), max_new_tokens, eos=eos,
                                                                            sampling=sampling, logprobs=output_logprobs, **lg)
        else:
            out, new_heads, *lps = self._generate_stepwise(vids, video_timestamps, id_lists, list(heads), max_new_tokens, eos,
                                                           sampling, stopping_criteria, output_logprobs, lgp, cons)
        for b in range(B):                       # the reference mutates `heads` in place (trace_mistral.py:342)
            heads[b] = int(new_heads[b])
        res, lp = self._padded(out, lps[0] if output_logprobs else None, eos if pad_token_id is None else pad_token_id)
        if not output_logprobs:
            return res
        return SimpleNamespace(sequences=res, logprobs=lp, heads=[int(h) for h in new_heads])

    @torch.no_grad()
    def generate_samples(self, inputs=None, images_or_videos=None, video_timestamps=None, n: int = 1, heads=None, max_new_tokens: int = 128,
                         temperature: Optional[float] = None, top_k: Optional[int] = None, top_p: Optional[float] = None, generation_config=None,
                         eos_token_id=None, pad_token_id: Optional[int] = None, modal_list=None, best_first: bool = True, retire_finished: bool = False,
                         **kwargs):
        """n sampled continuations of ONE prompt, ranked: the tower, the slot pool and the prefill run once (TraceEngine.generate_samples), the n
        rows decode as one batch with per-token log-probabilities.  Sampling arguments as generate(do_sample=True) (the seed comes from
        torch's default generator the same way); greedy parameters are a ValueError.  Returns `.sequences` [n, len] (padded as generate()),
        `.logprobs` float32 [n, len] (zero padded), `.scores` float64 [n] (each row's sum, accumulated in float64 from the float32 entries),
        `.order` (the decode-row index of each returned row) and `.heads`.  retire_finished: as generate() (a row keeps its Philox row index when others
        leave: the draws are the full batch's).  best_first: rows sorted by descending score, ties to the lower
        decode row; otherwise decode order."""
        if images_or_videos is None or video_timestamps is None:
            raise ValueError("generate_samples takes one video with its timestamps")
        ids = inputs if isinstance(inputs, torch.Tensor) else torch.tensor(inputs)
        if ids.dim() == 1:
            ids = ids.unsqueeze(0)
        if ids.shape[0] != 1 or len(images_or_videos) != 1 or len(video_timestamps) != 1:
            raise ValueError("generate_samples takes one prompt (B = 1); use generate() for a batch")
        if not isinstance(n, int) or isinstance(n, bool) or n < 1:
            raise ValueError(f"n must be a positive integer, got {n!r}")
        lgp = self._logits_params(kwargs.pop("repetition_penalty", None), kwargs.pop("no_repeat_ngram_size", None), kwargs.pop("min_new_tokens", None),
                                  generation_config)
        sampling = self._sampling_params(True, temperature, top_k, top_p, _ProcessorsOff(generation_config, self.generation_config), kwargs)
        eos, cons = self._eos_and_constraints(eos_token_id, kwargs, generation_config)
        if sampling is None:
            raise ValueError("generate_samples needs temperature > 0: greedy rows would all be identical")
        eng = self.engine
        head = 0 if heads is None else int(heads[0])
        eng.host_mode(False)
        self._live_kv = None
        x = self._as_frames(images_or_videos[0], (modal_list or ["video"])[0])
        out, new_heads, lps = eng.generate_samples(x, video_timestamps[0], ids[0].tolist(), head, n, max_new_tokens, eos=eos, sampling=sampling,
                                                   **({} if lgp is None else {"logits": lgp}), **({} if cons is None else {"constraints": cons}),
                                                   **({"retire_finished": True} if retire_finished else {}))
        scores = np.array([np.sum(np.asarray(r, np.float32), dtype=np.float64) for r in lps], np.float64)
        order = rank_samples(scores) if best_first else list(range(n))
        seq, lp = self._padded([out[r] for r in order], [lps[r] for r in order], eos if pad_token_id is None else pad_token_id)
        return SimpleNamespace(sequences=seq, logprobs=lp, scores=torch.from_numpy(scores[order].copy()),
                               order=[int(r) for r in order], heads=[int(new_heads[r]) for r in order])

    @torch.no_grad()
    def score(self, inputs=None, images_or_videos=None, video_timestamps=None, continuations=None, heads=None, modal_list=None, **kwargs):
        """How likely is each GIVEN continuation of ONE prompt?  (Multiple-choice scoring, ranking candidate captions or moments, the teacher-forced
        log-likelihood of a [time | score | caption] stream — what generate(output_logprobs=True) cannot say: it reports the tokens the model chose.)
        continuations: lists (or 1-D tensors) of global vocabulary ids over [text | <sync> | time | score]; heads: the head active for each one's
        first id — one int in a list for all of them (default [1], as generate's callers pass) or one per continuation.  Token i is scored under the
        head the fed ids c[0 .. i) lead to, from the hidden row that precedes it (include/trace_hip.h, trace_llm_score_append): all continuations
        run as appended rows behind the prompt's KV rows, up to 8 per pass, and their log-probabilities come from the fused head kernel — no
        [rows, vocabulary] logits exist at any point.  With enable_prefix_cache() on and a hit (same frame tensor, timestamps and ids through
        `<video>` as the previous generate() / score()), no tower pass and no prefill of the rows through `<video>` runs, and the entry stays
        valid afterwards: only rows behind it are rewritten.
        Returns a scoring.ScoreResult: `.logprobs` (a float32 array per continuation), `.heads` (the head of every token), `.scores` (float64 sums) and `.order`
        (continuation indices by descending score, ties to the lower index)."""
        if kwargs:
            raise TypeError(f"score() got unexpected arguments {sorted(kwargs)}")
        if images_or_videos is None or video_timestamps is None:
            raise ValueError("score takes one video with its timestamps")
        if continuations is None or len(continuations) < 1:
            raise ValueError("score needs at least one continuation")
        ids = inputs if isinstance(inputs, torch.Tensor) else torch.tensor(inputs)
        if ids.dim() == 1:
            ids = ids.unsqueeze(0)
        if ids.shape[0] != 1 or len(images_or_videos) != 1 or len(video_timestamps) != 1:
            raise ValueError("score takes one prompt (B = 1) with any number of continuations")
        conts = [[int(t) for t in (c.tolist() if isinstance(c, torch.Tensor) else c)] for c in continuations]
        hd = [1] if heads is None else [int(h) for h in heads]
        if len(hd) == 1:
            hd = hd * len(conts)
        if len(hd) != len(conts):
            raise ValueError("heads: one entry, or one per continuation")
        cfg, eng = self.config, self.engine
        conts = [scoring.check_continuation(cfg, c, h) for c, h in zip(conts, hd)]
        if cfg.mm_projector_type == "stc_connector":
            raise NotImplementedError("score runs on the TRACE path (time tokens per frame), not the legacy STC connector")
        eng.host_mode(False)
        self._live_kv = None
        raw = images_or_videos[0]
        modal = (modal_list or ["video"])[0]
        x = self._as_frames(raw, modal)
        prompt = ids[0].tolist()
        tail = None
        if self._prefix_cache and isinstance(raw, torch.Tensor):
            try:
                prefix, suffixes = split_questions([prompt])
            except ValueError:
                prefix, suffixes = None, [[]]
            if prefix is not None and len(suffixes[0]) > 0:
                ts = video_timestamps[0]
                key, hit, P0 = self._prefix_lookup(raw, ts, modal, prefix)
                if not hit:
                    eng.encode_video(x, ts)
                    P0 = eng.splice(prefix)
                    eng.prefill(0, P0)
                    eng.set_prefix_entry(key, P0)
                tail = eng.embed_rows(suffixes[0], want_output=True)        # the rows after <video> ride in front of every continuation: one pass
                P = P0 + tail.shape[0]
        if tail is None:
            eng.encode_video(x, video_timestamps[0])
            P, emb = eng.splice(prompt, want_output=True)
            emb = emb.clone()
            if P > 1:
                eng.prefill(0, P - 1, emb[: P - 1])
            tail = emb[P - 1:]
        lps, chains, sums = eng.score_continuations(0, P, tail, conts, hd)
        return scoring.ScoreResult(logprobs=lps, heads=chains, scores=sums, order=rank_samples(sums))

    # ---- what generate(), generate_samples() and score() share ----
    def _as_frames(self, x, modal):
        """an image stands for num_frames copies of itself (trace_arch.py:221); a video is taken as it is"""
        if modal != "image":
            return x
        nf = getattr(self.config, "num_frames", NUM_FRAMES)
        return x.unsqueeze(0).expand(nf, -1, -1, -1) if x.dim() == 3 else x.expand(nf, -1, -1, -1)

    def _eos_and_constraints(self, eos_token_id, kwargs, generation_config):
        """(eos, Constraints or None) of a generate() call, with HF's precedence (_pick; eos_token_id falls back to the config's).  eos_token_id is an
        int or a list: the first id is the engine's eos (-1 = none), the others become stop sequences of one id, duplicates dropped.
        bad_words_ids / suppress_tokens / begin_suppress_tokens / stop_sequences are popped from kwargs; as HF does, a bad word that is exactly
        [e] for an EOS id e is dropped.  ValueError outside the vocabulary or the device's bounds (sampling.check_constraints)."""
        gc = generation_config
        e = self._pick("eos_token_id", eos_token_id, gc, self.config.eos_token_id)
        if isinstance(e, torch.Tensor):
            e = e.tolist()
        eos_ids = []
        for t in ([] if e is None else e if isinstance(e, (list, tuple)) else [e]):
            if int(t) >= 0 and int(t) not in eos_ids:
                eos_ids.append(int(t))
        seqs = lambda name: [[int(t) for t in (w.tolist() if isinstance(w, torch.Tensor) else w)] for w in self._pick(name, kwargs.pop(name, None), gc, [])]
        flat = lambda name: [int(t) for t in self._pick(name, kwargs.pop(name, None), gc, [])]
        stops = seqs("stop_sequences")
        stops = [[t] for t in eos_ids[1:] if [t] not in stops] + stops
        bad = [w for w in seqs("bad_words_ids") if not (len(w) == 1 and w[0] in eos_ids)]
        cons = Constraints(stops, bad, flat("suppress_tokens"), flat("begin_suppress_tokens"))
        check_constraints(cons.stop_sequences, cons.bad_words_ids, cons.suppress_tokens, cons.begin_suppress_tokens, self.config.total_vocab)
        return (eos_ids[0] if eos_ids else -1), (None if cons.off else cons)

    def _padded(self, rows, lps, pad):
        """(ids int64 [B, n] padded with `pad` (0 when it is None or negative), log-probabilities float32 [B, n] zero padded, or None), on the device"""
        n = max(len(r) for r in rows)
        res = torch.full((len(rows), n), pad if pad is not None and pad >= 0 else 0, dtype=torch.long)
        lp = None if lps is None else torch.zeros((len(rows), n), dtype=torch.float32)
        for b, row in enumerate(rows):
            res[b, : len(row)] = torch.tensor(row, dtype=torch.long)
            if lp is not None:
                lp[b, : len(row)] = torch.from_numpy(np.asarray(lps[b], np.float32))
        return res.to(self.device), None if lp is None else lp.to(self.device)

    def _pick(self, name, value, generation_config, default=None):
        """HF's precedence: explicit argument > generation_config > the model's defaults > `default`"""
        if value is not None:
            return value
        for src in (generation_config, self.generation_config):
            v = None if src is None else src.get(name) if isinstance(src, dict) else getattr(src, name, None)
            if v is not None:
                return v
        return default

    # arguments of HF's generate() this build does not implement, with the value that means "off"
    _UNSUPPORTED = {"num_beams": 1, "num_return_sequences": 1, "repetition_penalty": 1.0}
    # HF's sampling warpers behind top_p, read from the keyword arguments, with the value that means "off" (None reads as off too).  The engine's
    # sampler applies them: an armed one that the engine does not list in `sampling_warpers` is refused like the names above, never dropped.
    _WARPERS = {"min_p": 0.0, "typical_p": 1.0, "epsilon_cutoff": 0.0, "eta_cutoff": 0.0}

    def _sampling_params(self, do_sample, temperature, top_k, top_p, generation_config, kwargs) -> Optional[SamplingParams]:
        """HF's precedence (_pick) for temperature / top_k / top_p and min_p / typical_p / epsilon_cutoff / eta_cutoff.  None = greedy."""
        gc = generation_config
        for name, off in self._UNSUPPORTED.items():
            v = self._pick(name, kwargs.get(name), gc)
            if v is not None and v != off:
                raise NotImplementedError(f"{name}={v!r} is not implemented on the MI355X path (only {name}={off!r})")
        warp, have = {}, getattr(self.engine, "sampling_warpers", ())
        for name, off in self._WARPERS.items():
            v = self._pick(name, kwargs.get(name), gc, off)
            if v != off and name not in have:
                raise NotImplementedError(f"{name}={v!r}: this model's engine does not implement `{name}` (only {name}={off!r})")
            warp[name] = float(v)
        do_sample, temperature = bool(self._pick("do_sample", do_sample, gc)), float(self._pick("temperature", temperature, gc))
        top_k, top_p = self._pick("top_k", top_k, gc, 0), float(self._pick("top_p", top_p, gc))
        check_sampling(temperature, top_k, top_p, **warp)
        if not do_sample or temperature <= 0:
            return None
        g = torch.randint(0, 1 << 32, (2,), dtype=torch.int64)        # torch's default generator: torch.manual_seed(s) reproduces a call
        return SamplingParams(temperature, int(top_k), top_p, (int(g[0]) << 32) | int(g[1]), **warp)

    def _logits_params(self, repetition_penalty, no_repeat_ngram_size, min_new_tokens, generation_config) -> Optional[LogitsParams]:
        """repetition_penalty / no_repeat_ngram_size / min_new_tokens with HF's precedence (_pick).  None = all three off (the decode step then
        is what it is without them).  ValueError outside HF's domains, and for an n-gram size above 64 (the device's bound)."""
        gc = generation_config
        lgp = LogitsParams(self._pick("repetition_penalty", repetition_penalty, gc, 1.0), self._pick("no_repeat_ngram_size", no_repeat_ngram_size, gc, 0),
                           self._pick("min_new_tokens", min_new_tokens, gc, 0))
        return None if lgp.off else lgp

    def _generate_stepwise(self, vids, timestamps, id_lists, heads, max_new, eos, sampling, stopping, logprobs=False, lgp=None, cons=None):
        """Stopping-criteria path: encode and prefill row by row, then TraceEngine.decode_stepwise with HF's StoppingCriteriaList as its callback.
        A row stops when ANY criterion fires for it; generate(inputs_embeds=...) hands the criteria the generated ids only (the reference calls
        super().generate with inputs_embeds, trace_mistral.py:301-312)."""
        eng, B = self.engine, len(vids)
        for b in range(B):
            eng.encode_video(vids[b], timestamps[b])
            eng.prefill(b, eng.splice(id_lists[b]))

        def fired(rows):
            n = max(len(x) for x in rows)
            gen = torch.tensor([x + [0] * (n - len(x)) for x in rows], dtype=torch.long)
            out = torch.zeros(B, dtype=torch.bool)
            for sc in stopping:
                r = sc(gen, None)
                out |= (r.view(-1).bool().cpu() if isinstance(r, torch.Tensor) else torch.full((B,), bool(r)))
            return out.tolist()
        return eng.decode_stepwise(range(B), heads, max_new, eos, sampling=sampling, logprobs=logprobs, logits=lgp, stopping=fired, constraints=cons)

    # ---- forward (trace_mistral.py:114-264) ----
    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None,
                labels=None, use_cache=None, images=None, times=None, scores=None, video_timestamps=None, heads=None, **kwargs):
        """Both forms of the reference's forward():
          * prefill form (`images=(videos, modal_list)`, `input_ids` with the modal placeholders): logits `[B, L, V']` fp32 for
            EVERY position of the spliced sequence (`heads` given: V' = V+1+Tv+Sv with everything outside the row's head at
            -inf; `heads=None`: the text|sync logits `[B, L, V+1]`, trace_mistral.py:190-193) and `past_key_values` = a handle
            on the KV slots the rows were prefilled into;
          * decode form (`input_ids [B, 1]` + that handle): the next-token embedding by id range (trace_arch.py:345-375), one
            decoder step, logits `[B, 1, V']`.
        Deviations, by design: `past_key_values` is an opaque handle (the cache lives in the engine, never in torch tensors);
        rows of a batch must splice to one length (the reference pads); `labels` / `inputs_embeds` are training / internal
        inputs and raise; in the decode form the active head is tracked on the device by the swap-token rule the reference's
        `prepare_inputs_for_generation` applies (trace_mistral.py:336-344), so a `heads` argument that disagrees with it raises."""
        if labels is not None or inputs_embeds is not None:
            raise NotImplementedError("forward(labels= / inputs_embeds=) belongs to training; outside the accelerated path")
        if input_ids is None:
            raise ValueError("input_ids is required")
        eng, cfg = self.engine, self.config
        ids = input_ids if input_ids.dim() == 2 else input_ids.unsqueeze(0)
        B = ids.shape[0]
        if past_key_values is not None:
            if not isinstance(past_key_values, _KVHandle) or past_key_values is not getattr(self, "_live_kv", None):
                raise ValueError("past_key_values must be the handle returned by the previous forward() of this model")
            if ids.shape[1] != 1 or B != past_key_values.B:
                raise ValueError("decode form takes input_ids [B, 1]")
            eng.feed([int(x) for x in ids[:, 0].tolist()])
            lg = eng.decode_steps(1, use_graph=False, want_logits=True)
            _, cur = eng.decode_read()
            if heads is not None and [int(h) for h in heads] != [int(h) for h in cur]:
                raise ValueError(f"heads={list(heads)} disagrees with the head state the fed tokens imply ({cur})")
            if heads is None:
                if any(cur):
                    raise ValueError("heads=None asks for text logits but the fed tokens switched a row to the time/score head")
                lg = lg[:, : cfg.vocab_size + 1]
            return SimpleNamespace(logits=lg.unsqueeze(1), past_key_values=past_key_values, loss=None, hidden_states=None,
                                   attentions=None)
        if images is None:
            raise NotImplementedError("text-only forward is outside the accelerated path")
        vids, modals = images
        hd = [0] * B if heads is None else [int(h) for h in heads]
        assert len(hd) == B                                                       # trace_mistral.py:245
        if B > eng.max_batch:
            raise ValueError(f"batch {B} exceeds the engine's max_batch {eng.max_batch}")
        rows = []
        for b in range(B):
            x = self._as_frames(vids[b], modals[b] if modals else "video")
            eng.encode_video(x, video_timestamps[b])
            trow = [int(i) for ev in (times[b] if times is not None else []) for i in self.model.time_tower.encode(ev)]
            srow = [int(i) for ev in (scores[b] if scores is not None else []) for i in self.model.score_tower.encode(ev)]
            L = eng.splice(ids[b].tolist(), trow, srow)
            hid = eng.prefill(b, L, want_hidden=True)
            rows.append(eng.head_logits(hid, hd[b]))
        if any(r.shape != rows[0].shape for r in rows):
            raise NotImplementedError("rows of one forward() batch must splice to the same length (no padding path in the engine)")
        logits = torch.stack(rows, 0)
        if heads is None:
            logits = logits[..., : cfg.vocab_size + 1]
        # arm the decode form: token selection stays with the caller (host mode), the cache stays in the engine.  The number of steps the
        # KV slots still have room for bounds the arming; a prompt that fills the context gets its logits and no decode form
        # (past_key_values=None) instead of an error after all the work is done.
        room = min(eng.max_new_tokens, eng.max_ctx - logits.shape[1])
        self._live_kv = None
        if room >= 1:
            eng.host_mode(True)
            try:
                eng.decode_begin(list(range(B)), hd, room, eos=-1)
            except Exception:
                eng.host_mode(False)
                raise
            self._live_kv = _KVHandle(B)
        return SimpleNamespace(logits=logits, past_key_values=self._live_kv, loss=None, hidden_states=None, attentions=None)

    __call__ = forward


class _ProcessorsOff:
    """A generation-config view for _sampling_params in which the logits processors this build implements read as off: generate() resolves them
    itself (_logits_params), and _sampling_params keeps refusing the name when it is called on its own."""

    def __init__(self, *srcs):
        self._srcs = [s for s in srcs if s is not None]

    def __getattr__(self, name):
        if name == "repetition_penalty":
            return 1.0
        for src in self._srcs:
            v = src.get(name) if isinstance(src, dict) else getattr(src, name, None)
            if v is not None:
                return v
        return None


def rank_samples(scores) -> List[int]:
    """decode-row indices by descending score; equal scores keep the lower row first"""
    return sorted(range(len(scores)), key=lambda r: (-float(scores[r]), r))


class _KVHandle:
    """`past_key_values` of this build: the KV cache stays inside the engine (slots 0..B-1); the handle only proves that the
    decode-form call follows the prefill-form call that filled them."""

    def __init__(self, B: int):
        self.B = B

    def get_seq_length(self, *a, **k):
        raise NotImplementedError("the KV cache is engine-resident")
