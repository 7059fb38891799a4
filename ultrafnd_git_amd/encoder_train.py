"""Trainable encoders: forward with saved activations + hand-written backward for BertTextEncoder / ClipVisualEncoder
(Tier-B backward; `TrainConfig.train_encoders`).

The reference keeps its encoder frozen (src/core_blocks/text_blocks.py:52 `.eval()`, :63 `inference_mode`) and trains on cached
features, so nothing here replaces a reference code path: it is the fine-tuning capability north_star's "forward/backward hot
path" of the encoders asks for.  Parity is against torch autograd over oracle/encoders_ref.py ("parity unpinned by the
reference": DESIGN.md section 2).

How it is built.
  * Parameters.  `groups()` lists the encoder's tensors in gradient-ready order (last layer first, embeddings last); the
    trainer lays them out in its ONE flat fp32 arena behind the head's, so the global-norm clip, AdamW and the gradient
    exchange stay single contiguous ranges.  q/k/v weights (and biases) of a layer are adjacent: the stacked (3H, H) operand is
    a view.  `bind()` re-points the encoder's master tensors at the arena.
  * Operands.  Every Linear has two bf16 copies of its fp32 master, W (forward, wgrad shape) and W^T (data gradient), re-cast
    after every optimizer step (`refresh_operands`: ufnd_cast_bf16 / ufnd_transpose_bf16 -- ~6 B per parameter per step).
  * Forward (`forward_train`).  The un-folded layer sequence (one LayerNorm kernel per LayerNorm), with what the backward needs
    kept per layer: the bf16 GEMM inputs, fused q|k|v rows, attention output and per-query log-sum-exp, the pre-LayerNorm sums
    (fp32), FFN1's pre-activations.
  * Backward (`backward`).  ONE chain per encoder (`_chain`) walks from d features down to the input; the parameter gradients
    are an option of that walk (`params`), which `backward` takes.  Per layer: LayerNorm backward (row kernel, two-stage
    parameter sums) -> for each Linear: transpose dy and x (dy's column sums = the bias gradient fall out of the same pass), weight gradient as the forward's NT kernel over
    the token dimension with split-K slabs, data gradient as the NT kernel on W^T with the residual-branch gradient or the
    activation derivative fused into its epilogue -> flash-style attention backward.  No atomics anywhere: gradients are
    run-to-run identical.
  * Dropout (HF train mode; BertTextEncoder.hidden_dropout_prob / .attention_probs_dropout_prob, ClipVisualEncoder.attention_dropout).
    Only here, never in the frozen paths.  At p = 0 a site runs exactly the launches it ran before dropout existed.  At p > 0:
    attention probabilities -> ufnd_attention_bf16_lse_dropout / _bwd_dropout; a text hidden site -> the dense GEMM writes its output
    without the residual and ufnd_dropout_residual_layernorm forms x + m o d and its LayerNorm (same launch count), the LayerNorm
    backward masks its bf16 output; the embeddings -> ufnd_layernorm_dropout, and the LayerNorm backward masks its dy.  No mask is
    stored: the kernels regenerate it from (seed, step) of `rng()` -- the trainer's step state (the head's), or the encoder's own,
    advanced by every forward_train -- and the site's tag (`text_tag`, `vision_tag`; ranges in csrc/common.hpp).
  * Input gradients (`forward_saved` / `input_grad`; explain.input_attribution).  The same `_chain` without the parameter gradients:
    `_wgrad` returns at once and `_ln_bwd` gets no scratch, so there are no transposes, no weight-gradient product, no second
    stream, LayerNorm backwards without dgamma / dbeta or a workspace, and nothing of the arena is looked up (the building blocks
    take parameter keys, not gradient tensors).  It goes one hop further -- to the raw embedding sums (text) and, through the patch
    embedding's data gradient and ufnd_vit_unpatchify_attribution, to the pixels (vision).  Dropout is off.  Its activations live in
    buffers of its own, so a forward_train waiting for its backward() is untouched.  It also runs on a FROZEN encoder (no arena bound): the bf16 W / W^T
    copies and the stacked q|k|v biases are then built from `enc._w` on first use and again when `weights_version` moves; nothing
    of the encoder is written either way."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib as L
from .encoders import ACT_GELU, ACT_NONE, ACT_QUICK_GELU, dropout_prob
from .state import StepStateBuffer

ACT_GELU_BWD, ACT_QUICK_GELU_BWD = 3, 4            # (ufnd_gemm_bf16_dgrad's epilogues; the forward's three are encoders.py's)

# dropout stream tags (csrc/common.hpp: UFND_TAG_TEXT, UFND_TAG_VISION)
TAG_TEXT, TAG_VISION = 256, 4096
SITE_ATTN, SITE_ATTN_OUT, SITE_FFN_OUT = 0, 1, 2
TAG_TEXT_EMB = TAG_TEXT


def text_tag(layer: int, site: int) -> int:
    """Text encoder layer `layer`, site SITE_ATTN (probabilities) / SITE_ATTN_OUT / SITE_FFN_OUT."""
    return TAG_TEXT + 1 + 3 * layer + site


def vision_tag(layer: int) -> int:
    """Visual encoder layer `layer`: the attention probabilities."""
    return TAG_VISION + layer


def _pad64(n: int) -> int:
    return (n + 63) // 64 * 64


def _cast_operands(m2: torch.Tensor, wb: torch.Tensor, wt: torch.Tensor, s) -> None:
    """bf16 W (wb) and W^T (wt) of one Linear from its fp32 master as a matrix (m2)."""
    L.check(L.lib().ufnd_cast_bf16(m2.data_ptr(), wb.data_ptr(), m2.numel(), s), "ufnd_cast_bf16")
    L.check(L.lib().ufnd_transpose_bf16(m2.data_ptr(), 1, m2.shape[0], m2.shape[1], m2.stride(0), wt.data_ptr(), wt.stride(0), m2.shape[0],
                                        None, None, 0, s), "ufnd_transpose_bf16")


class _Backprop:
    """Shared plumbing: parameter binding, operand copies, and the backward of one Linear / LayerNorm."""

    def __init__(self, enc):
        self.enc = enc
        self.arena = None
        self.prefix = ""
        self._ops: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}      # linear name -> (W bf16 (N, K), W^T bf16 (K, N))
        self._scratch: Dict[Tuple, dict] = {}
        self.saved: Optional[dict] = None
        self._refresh = None               # (device table, items, tiles, names left to the per-Linear path) of the grouped operand refresh
        self._views: Dict[Tuple, torch.Tensor] = {}
        self._pending_ln = None            # (job, scratch, buffer index) of a LayerNorm backward's deferred dgamma / dbeta finish (rides in the next Linear's finish launch)
        self._wg_side = None               # the stream of the weight-gradient products
        self._wg_open = False
        # weight-gradient products on a second stream beside the data-gradient chain (they are not on backward's critical path).  Measured
        # A/B/A/B on one box: 9.17 / 9.24 ms per step with it, 9.48 / 9.42 without -- once the host enqueue had come down to 4.6-5.2 ms per step
        # (memoised arena views); at 6.4 ms the events' extra 2-3 ms of host time made the step host-bound and the overlap invisible
        self.overlap_wgrad = True
        self.drop_state: Optional[StepStateBuffer] = None      # the trainer sets its own (the head's); None: rng() makes one
        self._owns_state = False
        self._drops: Dict[Tuple[int, float, int], object] = {}
        self.xsaved: Optional[dict] = None     # forward_saved's state (input_grad reads it; `saved` belongs to forward_train / backward)
        self._xbufs: Optional[Tuple[Tuple, dict]] = None       # its buffers: the latest shape only (a path chunk's are gigabytes)
        self._fz: Optional[dict] = None        # frozen encoder: operand copies and stacked biases of `weights_version`

    # ------------------------------------------------------------------ dropout
    def rng(self) -> StepStateBuffer:
        """The step state the dropout masks are drawn from (seed, step on the device): the trainer's, or this encoder's own (as
        DeepTruthClassifier.rng()), which every forward_train with dropout advances first."""
        if self.drop_state is None:
            self.drop_state = StepStateBuffer(self.enc.device, seed=torch.initial_seed() + 0xE7C)
            self._owns_state = True
        return self.drop_state

    def _begin_dropout(self) -> None:
        """Start of a training forward with dropout: a state of our own moves to the next step (forward and backward share it)."""
        st = self.rng()
        if self._owns_state:
            st.advance()

    def _drop(self, p: float, tag: int):
        """The ufnd_dropout descriptor of a site (memoised: one per site)."""
        st = self.rng()
        key = (st.ptr, p, tag)
        d = self._drops.get(key)
        if d is None:
            d = self._drops[key] = L.Dropout(st.ptr, p, tag)
        return d

    # ------------------------------------------------------------------ parameters
    def groups(self) -> List[List[Tuple[str, Tuple[int, ...]]]]:
        raise NotImplementedError

    def linears(self) -> Dict[str, Tuple[List[str], Optional[List[str]]]]:
        """linear name -> (weight keys stacked row-wise, bias keys or None)."""
        raise NotImplementedError

    def bind(self, arena, prefix: str) -> None:
        """Re-point the encoder's fp32 masters at their arena views (values preserved)."""
        self.arena, self.prefix = arena, prefix
        w = self.enc._w
        with torch.no_grad():
            for k in list(w):
                v = arena.view(prefix + k)
                v.copy_(w[k].to(v.device))
                w[k] = v
        self.enc._packed = None
        self.enc.weights_version += 1
        self._ops.clear()
        self._refresh = None
        self._views.clear()

    def _stacked(self, buf: torch.Tensor, keys: List[str]) -> torch.Tensor:
        """View of adjacent arena tensors as one matrix (q/k/v -> (3H, H)) or vector.  Memoised per buffer: a backward asks for ~400 of
        them, and building a view costs more host time than enqueueing the kernel that uses it."""
        ck = (buf.data_ptr(), keys[0], len(keys))
        v = self._views.get(ck)
        if v is None:
            v = self._views[ck] = self._stacked_view(buf, keys)
        return v

    def _stacked_view(self, buf: torch.Tensor, keys: List[str]) -> torch.Tensor:
        o0, s0 = self.arena.offsets[self.prefix + keys[0]]
        n = 0
        for k in keys:
            o, s = self.arena.offsets[self.prefix + k]
            if o != o0 + n:
                raise RuntimeError(f"{keys} are not adjacent in the arena")
            cnt = 1
            for dim in s:
                cnt *= int(dim)
            n += cnt
        rows = sum(self.arena.offsets[self.prefix + k][1][0] for k in keys)
        rest = tuple(s0[1:])
        return buf[o0:o0 + n].view((rows,) + rest)

    def _lk(self, i: int) -> dict:
        """The parameter names of layer i: the encoder's own table (memoised there)."""
        return self.enc.layer_keys(i)

    def master(self, keys: List[str]) -> torch.Tensor:
        """A master tensor (or adjacent ones stacked): the arena's view, or -- frozen -- the encoder's own."""
        if self.arena is not None:
            return self._stacked(self.arena.data, keys)
        return self.enc._w[keys[0]] if len(keys) == 1 else self._frozen()["stacked"][keys[0]]

    def grad(self, keys: List[str]) -> torch.Tensor:
        return self._stacked(self.arena.ensure_grad(), keys)

    def _frozen(self) -> dict:
        """No arena bound (a frozen encoder): {"ops": linear name -> (W bf16, W^T bf16), "stacked": first key -> the q|k|v biases as
        one vector}, cast from `enc._w` once per `weights_version`.  Reads the encoder only."""
        e = self.enc
        if self._fz is None or self._fz["version"] != e.weights_version:
            w, s = e._w, L.stream_ptr(e.device)
            ops, stacked = {}, {}
            for name, (wk, bk) in self.linears().items():
                m = w[wk[0]] if len(wk) == 1 else torch.cat([w[k] for k in wk], 0)
                m2 = m.reshape(m.shape[0], -1).contiguous()
                wb = torch.empty(m2.shape, dtype=torch.bfloat16, device=m2.device)
                wt = torch.empty((m2.shape[1], m2.shape[0]), dtype=torch.bfloat16, device=m2.device)
                _cast_operands(m2, wb, wt, s)
                ops[name] = (wb, wt)
                if bk is not None and len(bk) > 1:
                    stacked[bk[0]] = torch.cat([w[k] for k in bk], 0).contiguous()
            self._fz = {"version": e.weights_version, "ops": ops, "stacked": stacked}
        return self._fz

    def _op(self, name: str) -> Tuple[torch.Tensor, torch.Tensor]:
        """(W bf16, W^T bf16) of a Linear: the trained copies, or the frozen ones."""
        return self._ops[name] if self.arena is not None else self._frozen()["ops"][name]

    def _explain_bufs(self, key: Tuple, make) -> dict:
        key = key + (self.enc.device,)
        if self._xbufs is None or self._xbufs[0] != key:
            self._xbufs = None                 # (released before the next set is allocated)
            self._xbufs = (key, make())
        return self._xbufs[1]

    def _save_bufs(self, *shape: int) -> dict:
        """forward_train's buffers of a batch shape (kept: one set per shape seen)."""
        key = ("save",) + shape
        if key not in self._scratch:
            self._scratch[key] = self._make_bufs(*shape)
        return self._scratch[key]

    def _begin(self, train: bool) -> None:
        """Start of a forward: a bound encoder has its operand copies; only forward_saved may run without an arena (_frozen())."""
        self.enc._require_hip()
        if train and self.arena is None:
            raise RuntimeError("forward_train() before bind(): the parameter gradients go to an arena")
        if self.arena is not None and not self._ops:
            self.refresh_operands()

    def refresh_operands(self) -> None:
        """bf16 W and W^T of every Linear from the fp32 masters (after an optimizer step; captured-graph safe: fixed buffers): ONE
        grouped launch over all Linears whose shapes are multiples of 64 (every one of BERT-base / ViT-B), the two-launch form for
        the rest."""
        s = L.stream_ptr(self.enc.device)
        if self._refresh is None:
            items, rest, tile0 = [], [], 0
            for name, (wk, _) in self.linears().items():
                m = self.master(wk)
                m2 = m.reshape(m.shape[0], -1)
                if name not in self._ops:
                    self._ops[name] = (torch.empty(m2.shape, dtype=torch.bfloat16, device=m.device),
                                       torch.empty((m2.shape[1], m2.shape[0]), dtype=torch.bfloat16, device=m.device))
                wb, wt = self._ops[name]
                R, Cc = m2.shape
                ok = (R % 64 == 0 and Cc % 64 == 0 and m2.stride(1) == 1 and m2.stride(0) % 4 == 0 and m2.data_ptr() % 16 == 0 and
                      wb.data_ptr() % 16 == 0 and wt.data_ptr() % 16 == 0)
                if not ok:
                    rest.append(name)
                    continue
                it = L.RefreshItem()
                it.master, it.w, it.wt = m2.data_ptr(), wb.data_ptr(), wt.data_ptr()
                it.rows, it.cols, it.ld_master, it.ld_w, it.ld_wt, it.tile0 = R, Cc, m2.stride(0), wb.stride(0), wt.stride(0), tile0
                tile0 += (R // 64) * (Cc // 64)
                items.append(it)
            table = None
            if items:
                arr = (L.RefreshItem * len(items))(*items)
                table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self.enc.device)
            self._refresh = (table, len(items), tile0, rest)
        table, n_items, tiles, rest = self._refresh
        if n_items:
            L.check(L.lib().ufnd_refresh_operands(table.data_ptr(), n_items, tiles, s), "ufnd_refresh_operands")
        for name in rest:
            m = self.master(self.linears()[name][0])
            _cast_operands(m.reshape(m.shape[0], -1), *self._ops[name], s)

    # ------------------------------------------------------------------ scratch
    def _bwd_scratch(self, M: int, widths: Tuple[int, ...]) -> dict:
        key = (M,) + widths
        if key not in self._scratch:
            dev, Mp, wmax = self.enc.device, _pad64(M), max(widths)
            lib = L.lib()
            ws = max(lib.ufnd_gemm_bf16_wgrad_workspace_floats(a, b, Mp) for a in widths for b in widths if b % 64 == 0)
            two = lambda make: [make(), make()]
            # two buffer sets: the weight-gradient product of one Linear runs on a second stream while the main stream transposes the next
            # Linear's operands into the other set (busy[k] / ln_busy[k]: the event after which set k may be rewritten)
            self._scratch[key] = {
                "t1": two(lambda: torch.zeros(wmax, Mp, dtype=torch.bfloat16, device=dev)), "t2": two(lambda: torch.zeros(wmax, Mp, dtype=torch.bfloat16, device=dev)),
                "wg": two(lambda: torch.empty(max(1, ws), dtype=torch.float32, device=dev)),
                "cs": two(lambda: torch.empty(lib.ufnd_transpose_colsum_workspace_floats(Mp, wmax), dtype=torch.float32, device=dev)),
                "ln": two(lambda: torch.empty(lib.ufnd_layernorm_bwd_workspace_floats(M, self.enc.hidden), dtype=torch.float32, device=dev)),
                "flip": 0, "busy": [None, None], "ln_flip": 0, "ln_busy": [None, None]}
        return self._scratch[key]

    # ------------------------------------------------------------------ building blocks
    def _gemm(self, A, W, bias, out_bf16=None, out_f32=None, residual=None, act=ACT_NONE):
        self.enc._gemm(A, W, bias, out_bf16=out_bf16, out_f32=out_f32, residual=residual, act=act)

    def _dgrad(self, dy, wt, out_bf16=None, out_f32=None, residual=None, aux=None, act=ACT_NONE):
        """out (M, N) = dy (M, K) x wt (N, K)^T [x act'(aux)] [+ residual]."""
        M, K = dy.shape
        N = wt.shape[0]
        L.check(L.lib().ufnd_gemm_bf16_dgrad(dy.data_ptr(), wt.data_ptr(), L.ptr(residual), L.ptr(aux), L.ptr(out_bf16), L.ptr(out_f32), M, N, K,
                                             dy.stride(0), wt.stride(0), residual.stride(0) if residual is not None else 0,
                                             aux.stride(0) if aux is not None else 0, out_bf16.stride(0) if out_bf16 is not None else 0,
                                             out_f32.stride(0) if out_f32 is not None else 0, act, L.stream_ptr(dy.device)), "ufnd_gemm_bf16_dgrad")

    def _wgrad(self, sc: Optional[dict], dy, x, wk: List[str], bk: Optional[List[str]]) -> None:
        """The gradients of a Linear's weight (keys wk) and bias (keys bk, or None): dW (N, K) = dy (M, N)^T x (M, K); db (N) = column
        sums of dy.  (Overwrites: every step writes every gradient.)  sc None -- a pass without parameter gradients -- does nothing.  Three
        launches (ufnd_linear_wgrad): both transposes on the caller's stream -- dy may be overwritten behind them -- then the sliced NT
        product and one finish pass (which also carries a pending LayerNorm's dgamma / dbeta finish) on a SECOND stream, beside the
        data-gradient chain that continues on the caller's: the weight gradients are not on backward's critical path.  join_wgrad() ends it."""
        if sc is None:
            return
        dW, db = self.grad(wk), self.grad(bk) if bk is not None else None
        M, N = dy.shape
        K = x.shape[1]
        lib, dev = L.lib(), dy.device
        main = torch.cuda.current_stream(dev)
        if not self.overlap_wgrad:         # everything on the caller's stream (one buffer set)
            job, self._pending_ln = self._pending_ln, None
            L.check(lib.ufnd_linear_wgrad(dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), M, N, K, dW.reshape(N, -1).data_ptr(), L.ptr(db),
                                          sc["t1"][0].data_ptr(), sc["t2"][0].data_ptr(), sc["t1"][0].stride(0), sc["wg"][0].data_ptr(), sc["cs"][0].data_ptr(),
                                          C.byref(job[0]) if job is not None else None, L.WGRAD_ALL, main.cuda_stream), "ufnd_linear_wgrad")
            return
        if self._wg_side is None:
            self._wg_side = torch.cuda.Stream(device=dev)
        side = self._wg_side
        k = sc["flip"]
        sc["flip"] ^= 1
        if sc["busy"][k] is not None:
            main.wait_event(sc["busy"][k])             # the product that read this buffer set last
        t1, t2 = sc["t1"][k], sc["t2"][k]
        dW2 = dW.reshape(N, -1)
        job, self._pending_ln = self._pending_ln, None
        args = (dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), M, N, K, dW2.data_ptr(), L.ptr(db), t1.data_ptr(), t2.data_ptr(), t1.stride(0),
                sc["wg"][k].data_ptr(), sc["cs"][k].data_ptr(), C.byref(job[0]) if job is not None else None)
        L.check(lib.ufnd_linear_wgrad(*args, L.WGRAD_TRANSPOSE, main.cuda_stream), "ufnd_linear_wgrad")
        ev = torch.cuda.Event()
        ev.record(main)
        side.wait_event(ev)
        L.check(lib.ufnd_linear_wgrad(*args, L.WGRAD_PRODUCT, side.cuda_stream), "ufnd_linear_wgrad")
        done = torch.cuda.Event()
        done.record(side)
        sc["busy"][k] = done
        if job is not None:
            job[1]["ln_busy"][job[2]] = done            # the LayerNorm partials it finished may be overwritten after this
        self._wg_open = True

    def join_wgrad(self) -> None:
        """The caller's stream waits for every weight-gradient product started so far (end of a backward)."""
        if self._wg_open:
            torch.cuda.current_stream(self.enc.device).wait_stream(self._wg_side)
            self._wg_open = False

    def _flush_ln(self) -> None:
        """A deferred LayerNorm finish that no Linear picked up (the next kernel is another LayerNorm backward, or the backward ends)."""
        if self._pending_ln is not None:
            job, self._pending_ln = self._pending_ln, None
            L.check(L.lib().ufnd_row_partials_finish(C.byref(job[0]), 0, L.stream_ptr(self.enc.device)), "ufnd_row_partials_finish")
            job[1]["ln_busy"][job[2]] = None            # (stream order protects the buffer)

    def _ln_bwd(self, sc: Optional[dict], x, ldx, gk: List[str], bk: List[str], dy, dx_f32, dx_bf16, lddx, M, add=None, drop=None, where=0):
        """Backward of the LayerNorm with gain gk / bias bk (keys).  With a scratch its dgamma / dbeta go to the arena's gradients, their
        finish deferred (_pending_ln); sc None: the data gradient alone -- no dgamma / dbeta, no workspace, nothing deferred.
        drop (a ufnd_dropout) / where (L.LN_BWD_DROP_DXB or _DY): the mask of a dropout site at this LayerNorm."""
        H = self.enc.hidden
        dgamma = dbeta = ws = None
        if sc is not None:
            self._flush_ln()               # one pending job at a time: a LayerNorm backward right behind another one finishes the first here
            kk = sc["ln_flip"]
            sc["ln_flip"] ^= 1
            if sc["ln_busy"][kk] is not None:  # the finish (on the weight-gradient stream) that read this workspace last
                torch.cuda.current_stream(x.device).wait_event(sc["ln_busy"][kk])
                sc["ln_busy"][kk] = None
            dgamma, dbeta, ws = self.grad(gk), self.grad(bk), sc["ln"][kk]
        args = (x.data_ptr(), ldx, self.master(gk).data_ptr(), dy.data_ptr(), dy.stride(0), L.ptr(add), add.stride(0) if add is not None else 0,
                L.ptr(dx_f32), L.ptr(dx_bf16), lddx, L.ptr(dgamma), L.ptr(dbeta), L.ptr(ws), L.PARTIALS_DEFER if sc is not None else 0, M, H,
                self.enc.eps)
        if drop is None:
            L.check(L.lib().ufnd_layernorm_bwd(*args, L.stream_ptr(x.device)), "ufnd_layernorm_bwd")
        else:
            L.check(L.lib().ufnd_layernorm_bwd_dropout(*args, C.byref(drop), where, L.stream_ptr(x.device)), "ufnd_layernorm_bwd_dropout")
        if sc is None:
            return
        job = L.PartialsJob()
        job.part, job.nblk, job.H, job.out0, job.out1 = ws.data_ptr(), L.lib().ufnd_layernorm_bwd_blocks(M), H, dgamma.data_ptr(), dbeta.data_ptr()
        self._pending_ln = (job, sc, kk)

    def _attn_fwd(self, qkv, mask, ctx, lse, B, Lq, drop=None):
        args = (qkv.data_ptr(), L.ptr(mask), ctx.data_ptr(), lse.data_ptr(), B, Lq, self.enc.heads)
        if drop is None:
            L.check(L.lib().ufnd_attention_bf16_lse(*args, L.stream_ptr(qkv.device)), "ufnd_attention_bf16_lse")
        else:
            L.check(L.lib().ufnd_attention_bf16_lse_dropout(*args, C.byref(drop), L.stream_ptr(qkv.device)), "ufnd_attention_bf16_lse_dropout")

    def _attn_bwd(self, qkv, ctx, dctx, lse, mask, dqkv, ws, B, Lq, drop=None):
        args = (qkv.data_ptr(), ctx.data_ptr(), dctx.data_ptr(), lse.data_ptr(), L.ptr(mask), dqkv.data_ptr(), ws.data_ptr(), B, Lq, self.enc.heads)
        if drop is None:
            L.check(L.lib().ufnd_attention_bf16_bwd(*args, L.stream_ptr(qkv.device)), "ufnd_attention_bf16_bwd")
        else:
            L.check(L.lib().ufnd_attention_bf16_bwd_dropout(*args, C.byref(drop), L.stream_ptr(qkv.device)), "ufnd_attention_bf16_bwd_dropout")

    def _drop_ln(self, x, d, gamma, beta, y, out_bf16, out_f32, M, drop) -> None:
        """y = x + m o d, out = LayerNorm(y) (a post-LN residual site with dropout on the dense output d)."""
        e = self.enc
        L.check(L.lib().ufnd_dropout_residual_layernorm(x.data_ptr(), x.stride(0), d.data_ptr(), d.stride(0), gamma.data_ptr(), beta.data_ptr(),
                                                        y.data_ptr(), L.ptr(out_bf16), L.ptr(out_f32), M, e.hidden, e.eps, C.byref(drop),
                                                        L.stream_ptr(x.device)), "ufnd_dropout_residual_layernorm")


def _act(x: torch.Tensor, out: torch.Tensor, act: int) -> None:
    """bf16 activation over a whole tensor (training forward: FFN1 keeps its pre-activations AND their activation)."""
    L.check(L.lib().ufnd_act_bf16(x.data_ptr(), out.data_ptr(), x.numel(), act, L.stream_ptr(x.device)), "ufnd_act_bf16")


# =============================================================================================
class TextBackprop(_Backprop):
    """BertTextEncoder with a backward: BertModel (post-LN) -> masked mean-pool -> L2."""

    def groups(self):
        w, out = self.enc._w, []
        for i in reversed(range(self.enc.layers)):
            k = self._lk(i)
            for name in ("g2", "b2n", "w2", "b2", "w1", "b1", "g1", "b1n", "o_w", "o_b", "qkv_w", "qkv_b"):     # gradient-ready order inside the layer
                out.append([(key, tuple(w[key].shape)) for key in k[name]])
        for key in ("embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias", "embeddings.position_embeddings.weight",
                    "embeddings.token_type_embeddings.weight", "embeddings.word_embeddings.weight"):
            out.append([(key, tuple(w[key].shape))])
        return out

    def linears(self):
        d = {}
        for i in range(self.enc.layers):
            k = self._lk(i)
            d[f"{i}.qkv"], d[f"{i}.o"], d[f"{i}.w1"], d[f"{i}.w2"] = (k["qkv_w"], k["qkv_b"]), (k["o_w"], k["o_b"]), (k["w1"], k["b1"]), (k["w2"], k["b2"])
        return d

    def _make_bufs(self, B: int, Lq: int) -> dict:
        e, dev = self.enc, self.enc.device
        M, H, I = B * Lq, e.hidden, e.inter
        bf, f32 = dict(dtype=torch.bfloat16, device=dev), dict(dtype=torch.float32, device=dev)
        layers = [{"xb": torch.empty(M, H, **bf), "qkv": torch.empty(M, 3 * H, **bf), "ctx": torch.empty(M, H, **bf),
                   "lse": torch.empty(M, e.heads, **f32), "y1": torch.empty(M, H, **f32), "x1b": torch.empty(M, H, **bf),
                   "pre": torch.empty(M, I, **bf), "h": torch.empty(M, I, **bf), "y2": torch.empty(M, H, **f32)} for _ in range(e.layers)]
        return {"layers": layers, "s": torch.empty(M, H, **f32), "xf": torch.empty(M, H, **f32), "x1f": torch.empty(M, H, **f32),
                "xb_last": torch.empty(M, H, **bf), "hid": torch.empty(M, H, **f32), "feat": torch.empty(B, H, **f32),
                # backward
                "dx": torch.empty(M, H, **f32), "dyf": torch.empty(M, H, **f32), "dyb": torch.empty(M, H, **bf), "dx1": torch.empty(M, H, **f32),
                "dpre": torch.empty(M, I, **bf), "dctx": torch.empty(M, H, **bf), "dqkv": torch.empty(M, 3 * H, **bf),
                "aws": torch.empty(L.lib().ufnd_attention_bwd_workspace_floats(B, Lq, e.heads), **f32), "ds": torch.empty(M, H, **f32)}

    @torch.no_grad()
    def forward_train(self, input_ids: torch.Tensor, attention_mask: torch.Tensor) -> torch.Tensor:
        e = self.enc
        self._begin(True)
        ph = dropout_prob("hidden_dropout_prob", e.hidden_dropout_prob)
        pa = dropout_prob("attention_probs_dropout_prob", e.attention_probs_dropout_prob)
        if ph > 0.0 or pa > 0.0:
            self._begin_dropout()
        B, Lq = input_ids.shape
        self.saved = self._forward(self._save_bufs(B, Lq), input_ids, attention_mask, ph, pa)
        return self.saved["sv"]["feat"]

    @torch.no_grad()
    def forward_saved(self, input_ids: Optional[torch.Tensor], attention_mask: torch.Tensor, sums: Optional[torch.Tensor] = None) -> torch.Tensor:
        """forward_train without dropout, on a bound or a frozen encoder, keeping its activations for input_grad() in buffers of its
        own.  `sums` (B L, H) fp32: start from these raw embedding sums instead of embedding input_ids (a point of an integration
        path); they are read where they lie, also by input_grad()."""
        self._begin(False)
        B, Lq = attention_mask.shape
        sv = self._explain_bufs(("text", B, Lq), lambda: self._make_bufs(B, Lq))
        self.xsaved = self._forward(sv, input_ids, attention_mask, 0.0, 0.0, sums)
        return sv["feat"]

    def _forward(self, sv: dict, input_ids, attention_mask: torch.Tensor, ph: float, pa: float, sums: Optional[torch.Tensor] = None) -> dict:
        e = self.enc
        dev = e.device
        B, Lq = attention_mask.shape
        mask = attention_mask.to(dev, torch.int32).contiguous()
        M, H, w, s = B * Lq, e.hidden, e._w, L.stream_ptr(dev)
        lib = L.lib()
        if ph > 0.0 and "d" not in sv:
            sv["d"] = torch.empty(M, H, dtype=torch.float32, device=dev)       # a hidden site's dense output (without its residual)
        if sums is None:
            # embeddings: the raw sums are kept (their LayerNorm's backward needs its input)
            ids, sm = input_ids.to(dev, torch.int64).contiguous(), sv["s"]
            L.check(lib.ufnd_bert_embed(ids.data_ptr(), w["embeddings.word_embeddings.weight"].data_ptr(), w["embeddings.position_embeddings.weight"].data_ptr(),
                                        w["embeddings.token_type_embeddings.weight"].data_ptr(), None, None, None, sm.data_ptr(), B, Lq, H, e.vocab, e.eps, s),
                    "ufnd_bert_embed")
        else:
            ids, sm = None, sums
            if tuple(sm.shape) != (M, H) or sm.dtype != torch.float32 or not sm.is_contiguous() or sm.device != dev or sm.data_ptr() % 16:
                raise RuntimeError(f"sums: expected a contiguous 16-byte aligned fp32 ({M},{H}) tensor on {dev}")
        x_f, x_b = sv["xf"], sv["layers"][0]["xb"]
        if ph > 0.0:
            L.check(lib.ufnd_layernorm_dropout(sm.data_ptr(), H, w["embeddings.LayerNorm.weight"].data_ptr(), w["embeddings.LayerNorm.bias"].data_ptr(),
                                               x_b.data_ptr(), x_f.data_ptr(), M, H, e.eps, C.byref(self._drop(ph, TAG_TEXT_EMB)), s), "ufnd_layernorm_dropout")
        else:
            e._ln(sm, H, w["embeddings.LayerNorm.weight"], w["embeddings.LayerNorm.bias"], x_b, x_f, M, H, e.eps)
        for i, a in enumerate(sv["layers"]):
            k = self._lk(i)
            wqkv, wo, w1, w2 = self._op(f"{i}.qkv")[0], self._op(f"{i}.o")[0], self._op(f"{i}.w1")[0], self._op(f"{i}.w2")[0]
            self._gemm(a["xb"], wqkv, self.master(k["qkv_b"]), out_bf16=a["qkv"])
            self._attn_fwd(a["qkv"], mask, a["ctx"], a["lse"], B, Lq, self._drop(pa, text_tag(i, SITE_ATTN)) if pa > 0.0 else None)
            if ph > 0.0:
                self._gemm(a["ctx"], wo, self.master(k["o_b"]), out_f32=sv["d"])
                self._drop_ln(x_f, sv["d"], self.master(k["g1"]), self.master(k["b1n"]), a["y1"], a["x1b"], sv["x1f"], M,
                              self._drop(ph, text_tag(i, SITE_ATTN_OUT)))
            else:
                self._gemm(a["ctx"], wo, self.master(k["o_b"]), out_f32=a["y1"], residual=x_f)
                e._ln(a["y1"], H, self.master(k["g1"]), self.master(k["b1n"]), a["x1b"], sv["x1f"], M, H, e.eps)
            self._gemm(a["x1b"], w1, self.master(k["b1"]), out_bf16=a["pre"])
            _act(a["pre"], a["h"], ACT_GELU)
            nxt_b = sv["layers"][i + 1]["xb"] if i + 1 < e.layers else sv["xb_last"]
            if ph > 0.0:
                self._gemm(a["h"], w2, self.master(k["b2"]), out_f32=sv["d"])
                self._drop_ln(sv["x1f"], sv["d"], self.master(k["g2"]), self.master(k["b2n"]), a["y2"], nxt_b, x_f, M,
                              self._drop(ph, text_tag(i, SITE_FFN_OUT)))
            else:
                self._gemm(a["h"], w2, self.master(k["b2"]), out_f32=a["y2"], residual=sv["x1f"])
                e._ln(a["y2"], H, self.master(k["g2"]), self.master(k["b2n"]), nxt_b, x_f, M, H, e.eps)
        sv["hid"].copy_(x_f)
        L.check(lib.ufnd_masked_meanpool_l2(sv["hid"].data_ptr(), mask.data_ptr(), sv["feat"].data_ptr(), B, Lq, H, s), "ufnd_masked_meanpool_l2")
        return {"B": B, "L": Lq, "ids": ids, "mask": mask, "sv": sv, "ph": ph, "pa": pa, "s": sm}

    def _chain(self, st: dict, dfeat: torch.Tensor, params: bool) -> None:
        """The backward of the batch kept in `st`, from d / d features (B, H) down to the raw embedding sums (sv["ds"]).  params: also
        every parameter gradient (weight gradients beside the chain, deferred LayerNorm sums, the embedding tables), into the arena's
        gradient buffer; without them no launch but the data gradients', and nothing of the arena is touched."""
        e = self.enc
        B, Lq, ids, mask, sv, ph, pa = st["B"], st["L"], st["ids"], st["mask"], st["sv"], st["ph"], st["pa"]
        M, H = B * Lq, e.hidden
        DXB = L.LN_BWD_DROP_DXB
        sc = self._bwd_scratch(M, (H, 3 * H, e.inter)) if params else None
        s = L.stream_ptr(e.device)
        dfeat = L.f32c(dfeat.to(e.device))
        L.check(L.lib().ufnd_masked_meanpool_l2_bwd(sv["hid"].data_ptr(), mask.data_ptr(), dfeat.data_ptr(), sv["dx"].data_ptr(), B, Lq, H, s),
                "ufnd_masked_meanpool_l2_bwd")
        dx = sv["dx"]
        for i in reversed(range(e.layers)):
            a, k = sv["layers"][i], self._lk(i)
            # output.LayerNorm, output.dense, GELU, intermediate.dense
            self._ln_bwd(sc, a["y2"], H, k["g2"], k["b2n"], dx, sv["dyf"], sv["dyb"], H, M,
                         drop=self._drop(ph, text_tag(i, SITE_FFN_OUT)) if ph > 0.0 else None, where=DXB)
            self._wgrad(sc, sv["dyb"], a["h"], k["w2"], k["b2"])
            self._dgrad(sv["dyb"], self._op(f"{i}.w2")[1], out_bf16=sv["dpre"], aux=a["pre"], act=ACT_GELU_BWD)
            self._wgrad(sc, sv["dpre"], a["x1b"], k["w1"], k["b1"])
            self._dgrad(sv["dpre"], self._op(f"{i}.w1")[1], out_f32=sv["dx1"], residual=sv["dyf"])
            # attention.output.LayerNorm, attention.output.dense, attention, q/k/v
            self._ln_bwd(sc, a["y1"], H, k["g1"], k["b1n"], sv["dx1"], sv["dyf"], sv["dyb"], H, M,
                         drop=self._drop(ph, text_tag(i, SITE_ATTN_OUT)) if ph > 0.0 else None, where=DXB)
            self._wgrad(sc, sv["dyb"], a["ctx"], k["o_w"], k["o_b"])
            self._dgrad(sv["dyb"], self._op(f"{i}.o")[1], out_bf16=sv["dctx"])
            self._attn_bwd(a["qkv"], a["ctx"], sv["dctx"], a["lse"], mask, sv["dqkv"], sv["aws"], B, Lq,
                           self._drop(pa, text_tag(i, SITE_ATTN)) if pa > 0.0 else None)
            self._wgrad(sc, sv["dqkv"], a["xb"], k["qkv_w"], k["qkv_b"])
            self._dgrad(sv["dqkv"], self._op(f"{i}.qkv")[1], out_f32=dx, residual=sv["dyf"])
        # embeddings: LayerNorm backward to the raw sums (forward_saved's may be the caller's), then the three tables
        ek = "embeddings."
        self._ln_bwd(sc, st["s"], H, [ek + "LayerNorm.weight"], [ek + "LayerNorm.bias"], dx, sv["ds"], None, H, M,
                     drop=self._drop(ph, TAG_TEXT_EMB) if ph > 0.0 else None, where=L.LN_BWD_DROP_DY)
        if params:
            L.check(L.lib().ufnd_bert_embed_bwd(ids.data_ptr(), sv["ds"].data_ptr(), self.grad([ek + "word_embeddings.weight"]).data_ptr(),
                                                self.grad([ek + "position_embeddings.weight"]).data_ptr(), self.grad([ek + "token_type_embeddings.weight"]).data_ptr(),
                                                B, Lq, H, e.vocab, e.max_position, self.master([ek + "token_type_embeddings.weight"]).shape[0], s), "ufnd_bert_embed_bwd")
            self._flush_ln()               # (the embedding LayerNorm's dgamma / dbeta: no Linear follows it)
            self.join_wgrad()

    @torch.no_grad()
    def input_grad(self, dfeat: torch.Tensor) -> torch.Tensor:
        """ds (B L, H): the gradient of the raw embedding sums (`xsaved["s"]`, before the embedding LayerNorm) from d / d features
        (B, H), for the batch of the last forward_saved(): the chain without a single parameter gradient; rows of masked tokens
        come out as zero.  The returned buffer is rewritten by the next call of the same shape."""
        if self.xsaved is None:
            raise RuntimeError("input_grad() without forward_saved()")
        self._chain(self.xsaved, dfeat, False)
        return self.xsaved["sv"]["ds"]

    @torch.no_grad()
    def backward(self, dfeat: torch.Tensor) -> None:
        """Gradients of every encoder parameter (into the arena's gradient buffer) from d loss / d features (B, H)."""
        if self.saved is None:
            raise RuntimeError("backward() without forward_train()")
        self._chain(self.saved, dfeat, True)


# =============================================================================================
class VisualBackprop(_Backprop):
    """ClipVisualEncoder with a backward: CLIP ViT (pre-LN) -> pooled CLS -> projection -> frame pooling."""

    V = "vision_model."

    def groups(self):
        w, V, out = self.enc._w, self.V, []
        for key in ("visual_projection.weight", V + "post_layernorm.weight", V + "post_layernorm.bias"):
            out.append([(key, tuple(w[key].shape))])
        for i in reversed(range(self.enc.layers)):
            k = self._lk(i)
            for name in ("w2", "b2", "w1", "b1", "g2", "b2n", "o_w", "o_b", "qkv_w", "qkv_b", "g1", "b1n"):
                out.append([(key, tuple(w[key].shape)) for key in k[name]])
        for key in (V + "pre_layrnorm.weight", V + "pre_layrnorm.bias", V + "embeddings.position_embedding.weight", V + "embeddings.class_embedding",
                    V + "embeddings.patch_embedding.weight"):
            out.append([(key, tuple(w[key].shape))])
        return out

    def linears(self):
        d = {"proj": (["visual_projection.weight"], None), "patch": ([self.V + "embeddings.patch_embedding.weight"], None)}
        for i in range(self.enc.layers):
            k = self._lk(i)
            d[f"{i}.qkv"], d[f"{i}.o"], d[f"{i}.w1"], d[f"{i}.w2"] = (k["qkv_w"], k["qkv_b"]), (k["o_w"], k["o_b"]), (k["w1"], k["b1"]), (k["w2"], k["b2"])
        return d

    def _make_bufs(self, B: int, Fr: int) -> dict:
        e, dev = self.enc, self.enc.device
        N, T, H, I = B * Fr, e.n_patches + 1, e.hidden, e.inter
        M, NP = N * T, N * e.n_patches
        bf, f32 = dict(dtype=torch.bfloat16, device=dev), dict(dtype=torch.float32, device=dev)
        layers = [{"xin": torch.empty(M, H, **f32), "h1b": torch.empty(M, H, **bf), "qkv": torch.empty(M, 3 * H, **bf), "ctx": torch.empty(M, H, **bf),
                   "lse": torch.empty(M, e.heads, **f32), "xmid": torch.empty(M, H, **f32), "h2b": torch.empty(M, H, **bf),
                   "pre": torch.empty(M, I, **bf), "m": torch.empty(M, I, **bf)} for _ in range(e.layers)]
        Np = _pad64(N)
        return {"layers": layers, "patches": torch.empty(NP, 3 * e.patch ** 2, **bf), "pe": torch.empty(NP, H, **f32),
                "s": torch.empty(M, H, **f32), "xout": torch.empty(M, H, **f32), "pooled_b": torch.zeros(Np, H, **bf),
                "pooled_f": torch.empty(N, H, **f32), "e": torch.empty(N, e.proj, **f32), "feat": torch.empty(B, e.proj, **f32),
                # backward
                "de": torch.empty(N, e.proj, **f32), "de_b": torch.zeros(Np, e.proj, **bf), "dpool": torch.empty(Np, H, **f32),
                "dx": torch.empty(M, H, **f32), "dxb": torch.empty(M, H, **bf), "dh": torch.empty(M, H, **f32),
                "dmid": torch.empty(M, H, **f32), "dmidb": torch.empty(M, H, **bf), "dpre": torch.empty(M, I, **bf),
                "dctx": torch.empty(M, H, **bf), "dqkv": torch.empty(M, 3 * H, **bf), "ds": torch.empty(M, H, **f32),
                "dpe": torch.empty(NP, H, **bf), "aws": torch.empty(L.lib().ufnd_attention_bwd_workspace_floats(N, T, e.heads), **f32)}

    def _frames5(self, frames: torch.Tensor) -> torch.Tensor:
        if frames.dim() == 4:
            frames = frames[:, None]
        e = self.enc
        if frames.dim() != 5 or tuple(frames.shape[2:]) != (3, e.image, e.image):
            raise RuntimeError(f"frames: expected (B,F,3,{e.image},{e.image}), got {tuple(frames.shape)}")
        return frames

    @torch.no_grad()
    def forward_train(self, frames: torch.Tensor) -> torch.Tensor:
        e = self.enc
        self._begin(True)
        frames = self._frames5(frames)
        pa = dropout_prob("attention_dropout", e.attention_dropout)
        if pa > 0.0:
            self._begin_dropout()
        self.saved = self._forward(self._save_bufs(*frames.shape[:2]), frames, pa)
        return self.saved["sv"]["feat"]

    @torch.no_grad()
    def forward_saved(self, frames: torch.Tensor) -> torch.Tensor:
        """forward_train without dropout, on a bound or a frozen encoder, keeping its activations for input_grad() in buffers of its
        own."""
        self._begin(False)
        frames = self._frames5(frames)
        B, Fr = frames.shape[:2]

        def make():
            sv = self._make_bufs(B, Fr)
            sv["dpatch"] = torch.empty(B * Fr * self.enc.n_patches, 3 * self.enc.patch ** 2, dtype=torch.float32, device=self.enc.device)
            return sv
        self.xsaved = self._forward(self._explain_bufs(("vision", B, Fr), make), frames, 0.0)
        return self.xsaved["sv"]["feat"]

    def _forward(self, sv: dict, frames: torch.Tensor, pa: float) -> dict:
        e = self.enc
        dev = e.device
        B, Fr = frames.shape[:2]
        fr = L.f32c(frames.to(dev)).view(B * Fr, 3, e.image, e.image)
        N, T, H, w, V = B * Fr, e.n_patches + 1, e.hidden, e._w, self.V
        M, s, lib = N * T, L.stream_ptr(dev), L.lib()
        L.check(lib.ufnd_vit_patchify(fr.data_ptr(), sv["patches"].data_ptr(), N, e.image, e.patch, s), "ufnd_vit_patchify")
        self._gemm(sv["patches"], self._op("patch")[0], None, out_f32=sv["pe"])
        L.check(lib.ufnd_vit_assemble(sv["pe"].data_ptr(), w[V + "embeddings.class_embedding"].data_ptr(), w[V + "embeddings.position_embedding.weight"].data_ptr(),
                                      None, None, sv["s"].data_ptr(), None, None, N, e.n_patches, H, e.eps, s), "ufnd_vit_assemble")
        x = sv["layers"][0]["xin"]
        e._ln(sv["s"], H, w[V + "pre_layrnorm.weight"], w[V + "pre_layrnorm.bias"], None, x, M, H, e.eps)
        for i, a in enumerate(sv["layers"]):
            k = self._lk(i)
            wqkv, wo, w1, w2 = self._op(f"{i}.qkv")[0], self._op(f"{i}.o")[0], self._op(f"{i}.w1")[0], self._op(f"{i}.w2")[0]
            e._ln(a["xin"], H, self.master(k["g1"]), self.master(k["b1n"]), a["h1b"], None, M, H, e.eps)
            self._gemm(a["h1b"], wqkv, self.master(k["qkv_b"]), out_bf16=a["qkv"])
            self._attn_fwd(a["qkv"], None, a["ctx"], a["lse"], N, T, self._drop(pa, vision_tag(i)) if pa > 0.0 else None)
            self._gemm(a["ctx"], wo, self.master(k["o_b"]), out_f32=a["xmid"], residual=a["xin"])
            e._ln(a["xmid"], H, self.master(k["g2"]), self.master(k["b2n"]), a["h2b"], None, M, H, e.eps)
            self._gemm(a["h2b"], w1, self.master(k["b1"]), out_bf16=a["pre"])
            _act(a["pre"], a["m"], ACT_QUICK_GELU)
            nxt = sv["layers"][i + 1]["xin"] if i + 1 < e.layers else sv["xout"]
            self._gemm(a["m"], w2, self.master(k["b2"]), out_f32=nxt, residual=a["xmid"])
        e._ln(sv["xout"], T * H, w[V + "post_layernorm.weight"], w[V + "post_layernorm.bias"], sv["pooled_b"], sv["pooled_f"], N, H, e.eps)
        self._gemm(sv["pooled_b"][:N], self._op("proj")[0], None, out_f32=sv["e"])
        L.check(lib.ufnd_l2norm_frames(sv["e"].data_ptr(), sv["feat"].data_ptr(), B, Fr, e.proj, s), "ufnd_l2norm_frames")
        return {"B": B, "F": Fr, "sv": sv, "pa": pa}

    def _chain(self, st: dict, dfeat: torch.Tensor, params: bool) -> None:
        """The backward of the batch kept in `st`, from d / d features (B, proj) down to the patch embedding's output (sv["dpe"]).
        params: also every parameter gradient, the patch embedding's weight included, into the arena's gradient buffer; without them
        no launch but the data gradients', nothing of the arena is touched, and the walk goes one Linear further, to the patch
        matrix (sv["dpatch"])."""
        e = self.enc
        B, Fr, sv, pa, V = st["B"], st["F"], st["sv"], st["pa"], self.V
        N, T, H = B * Fr, e.n_patches + 1, e.hidden
        M = N * T
        sc = scp = sch = None
        if params:
            sc = self._bwd_scratch(M, (H, 3 * H, e.inter))
            scp = self._bwd_scratch(N * e.n_patches, (H, 3 * e.patch ** 2))
            sch = self._bwd_scratch(N, (e.proj, H))
        s, lib = L.stream_ptr(e.device), L.lib()
        dfeat = L.f32c(dfeat.to(e.device))
        # frame pooling, projection (bias-free), post-LayerNorm on the CLS rows
        L.check(lib.ufnd_l2norm_frames_bwd(sv["e"].data_ptr(), dfeat.data_ptr(), sv["de"].data_ptr(), B, Fr, e.proj, s), "ufnd_l2norm_frames_bwd")
        de_b = sv["de_b"][:N]
        de_b.copy_(sv["de"])
        self._wgrad(sch, de_b, sv["pooled_b"][:N], ["visual_projection.weight"], None)
        self._dgrad(de_b, self._op("proj")[1], out_f32=sv["dpool"][:N])
        dx = sv["dx"]
        dx.zero_()                       # only the CLS rows of the last layer's output carry a gradient
        sv["dxb"].zero_()
        self._ln_bwd(sch, sv["xout"], T * H, [V + "post_layernorm.weight"], [V + "post_layernorm.bias"], sv["dpool"][:N], dx, sv["dxb"], T * H, N)
        for i in reversed(range(e.layers)):
            a, k = sv["layers"][i], self._lk(i)
            # MLP branch: x_out = x_mid + fc2(quick_gelu(fc1(LN2(x_mid))))
            self._wgrad(sc, sv["dxb"], a["m"], k["w2"], k["b2"])
            self._dgrad(sv["dxb"], self._op(f"{i}.w2")[1], out_bf16=sv["dpre"], aux=a["pre"], act=ACT_QUICK_GELU_BWD)
            self._wgrad(sc, sv["dpre"], a["h2b"], k["w1"], k["b1"])
            self._dgrad(sv["dpre"], self._op(f"{i}.w1")[1], out_f32=sv["dh"])
            self._ln_bwd(sc, a["xmid"], H, k["g2"], k["b2n"], sv["dh"], sv["dmid"], sv["dmidb"], H, M, add=dx)
            # attention branch: x_mid = x_in + out_proj(attn(qkv(LN1(x_in))))
            self._wgrad(sc, sv["dmidb"], a["ctx"], k["o_w"], k["o_b"])
            self._dgrad(sv["dmidb"], self._op(f"{i}.o")[1], out_bf16=sv["dctx"])
            self._attn_bwd(a["qkv"], a["ctx"], sv["dctx"], a["lse"], None, sv["dqkv"], sv["aws"], N, T,
                           self._drop(pa, vision_tag(i)) if pa > 0.0 else None)
            self._wgrad(sc, sv["dqkv"], a["h1b"], k["qkv_w"], k["qkv_b"])
            self._dgrad(sv["dqkv"], self._op(f"{i}.qkv")[1], out_f32=sv["dh"])
            self._ln_bwd(sc, a["xin"], H, k["g1"], k["b1n"], sv["dh"], dx, sv["dxb"], H, M, add=sv["dmid"])
        # pre-LayerNorm, token assembly, patch embedding
        self._ln_bwd(sc, sv["s"], H, [V + "pre_layrnorm.weight"], [V + "pre_layrnorm.bias"], dx, sv["ds"], None, H, M)
        dcls, dpos = (self.grad([V + "embeddings.class_embedding"]), self.grad([V + "embeddings.position_embedding.weight"])) if params else (None, None)
        L.check(lib.ufnd_vit_assemble_bwd(sv["ds"].data_ptr(), L.ptr(dcls), L.ptr(dpos), sv["dpe"].data_ptr(), N, e.n_patches, H, s), "ufnd_vit_assemble_bwd")
        if params:
            self._wgrad(scp, sv["dpe"], sv["patches"], [V + "embeddings.patch_embedding.weight"], None)
            self._flush_ln()
            self.join_wgrad()
        else:
            self._dgrad(sv["dpe"], self._op("patch")[1], out_f32=sv["dpatch"])

    @torch.no_grad()
    def patch_grad(self, dfeat: torch.Tensor) -> torch.Tensor:
        """(B F P, 3 p^2) fp32: the gradient of the patch matrix (ufnd_vit_patchify's layout) from d / d features (B, proj), for the
        batch of the last forward_saved(): the chain without a single parameter gradient, on through the patch rows of the
        token-assembly backward and the patch embedding's data gradient.  Rewritten by the next call of the shape."""
        if self.xsaved is None:
            raise RuntimeError("patch_grad() without forward_saved()")
        self._chain(self.xsaved, dfeat, False)
        return self.xsaved["sv"]["dpatch"]

    @torch.no_grad()
    def input_grad(self, dfeat: torch.Tensor) -> torch.Tensor:
        """dframes (B, F, 3, S, S): patch_grad() laid back into frame layout (ufnd_vit_unpatchify_attribution)."""
        dp = self.patch_grad(dfeat)
        e, st = self.enc, self.xsaved
        out = torch.empty(st["B"], st["F"], 3, e.image, e.image, dtype=torch.float32, device=e.device)
        L.check(L.lib().ufnd_vit_unpatchify_attribution(dp.data_ptr(), None, None, out.data_ptr(), None, None, st["B"] * st["F"], e.image, e.patch,
                                                        L.stream_ptr(e.device)), "ufnd_vit_unpatchify_attribution")
        return out

    @torch.no_grad()
    def backward(self, dfeat: torch.Tensor) -> None:
        """Gradients of every encoder parameter (into the arena's gradient buffer) from d loss / d features (B, proj)."""
        if self.saved is None:
            raise RuntimeError("backward() without forward_train()")
        self._chain(self.saved, dfeat, True)
