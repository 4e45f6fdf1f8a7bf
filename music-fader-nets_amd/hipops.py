"""Tensor-level wrappers over the C ABI (include/fadernets.h).

PyTorch is only the owner of device memory and of the current HIP stream here: each method checks
dtype / device / layout, takes ``data_ptr()`` and calls the HIP kernel on
``torch.cuda.current_stream()``.  No method has a CPU or eager-torch fallback; a missing library or
a non-zero return code raises.
"""
import ctypes as C

import torch

from . import _lib, arith


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk(t, dtype=torch.float32, name="tensor"):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU (got %s): the HIP path has no CPU fallback" % (name, t.device))
    if t.dtype != dtype:
        raise RuntimeError("%s must be %s, got %s" % (name, dtype, t.dtype))


def _mat(t, name):
    """2-D view with unit inner stride -> (ptr, rows, cols, ld)."""
    _chk(t, name=name)
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise RuntimeError("%s must be 2-D with contiguous rows, got shape %s strides %s" % (name, tuple(t.shape), t.stride()))
    ld = t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))
    return _p(t), t.shape[0], t.shape[1], ld


def _dense(t, dtype=torch.float32, name="tensor"):
    _chk(t, dtype, name)
    if t is not None and not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)
    return _p(t)


class HipOps:
    """The product backend: every method is one C-ABI call on the current stream."""

    name = "hip"

    def __init__(self, device):
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("HipOps needs a GPU device")
        self._ws = {}
        self._retired = []
        self.cell_variant = 0     # FnGruCell.variant (tuning / tests)
        self.dw_x6 = arith.default() == arith.BF16X6        # arithmetic of the deep products (the package default; a model sets its own choice: arith.py): True = exact bf16 triple splits on the bf16 MFMA (FN_GEMM_BF16X6, FN_GRU_BF16X6), False = fp32 MFMA
        self.x6_wide = True       # with dw_x6: 128 x 256 output tiles (FN_GEMM_X6_WIDE) where the product has >= 256 columns - with TWICE the K ranges the caller asked for (the same number of workgroups); False: 128 x 128 tiles
        self.nt_x6 = True         # with dw_x6: the big Linear-forward / dX products (whole 128 x 128 tiles, K % 32 == 0) on the bf16 x 6 kernel too; False: fp32 MFMA (A/B measurements)
        self.x6_per_tile = False  # A/B, tests: the producer / consumer bf16 x 6 kernels as one workgroup per output tile / (tile, K range) item (round 6: one per CU walking its items)
        self.cell_x6_rows = 2048  # ... from this many rows on (tests: 0 = wherever the kernel takes the shape)
        self.cell_x6 = True       # with dw_x6: the large-batch decode cells (fn_gru_cell_f32) on the bf16 x 6 producer / consumer kernel (gru_cell_x6_kernel); False: fp32 MFMA cells
        self.x6_perwave = False   # with dw_x6: the round-5 weight-gradient kernel in which every wavefront splits its own operands (FN_GEMM_X6_PERWAVE; A/B measurements, tests)
        self.bwd_x6 = True        # with dw_x6: the backward scans on the bf16 x 6 kernel too (False: fp32 MFMA backward scans; A/B measurements, tests)
        self.variant = 0          # FnGruFwd.variant of every scan launch (tuning / tests only; results do not depend on it)
        self.lane = ""            # scratch namespace: kernels enqueued on different streams must not share workspaces

    # -- plumbing -------------------------------------------------------------------------------
    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def workspace(self, nbytes, tag="ws"):
        """Grow-only scratch buffer per tag.  A captured hipGraph holds the raw pointer it was captured with, so a buffer that is
        outgrown is RETIRED (kept alive for the lifetime of this object), never freed: graphs of smaller batch shapes keep replaying
        on their own scratch."""
        tag = self.lane + tag
        cur = self._ws.get(tag)
        if cur is None or cur.numel() * 4 < nbytes:
            if cur is not None:
                self._retired.append(cur)
            cur = torch.empty((max(nbytes, 4) + 3) // 4, dtype=torch.float32, device=self.device)
            self._ws[tag] = cur
        return cur

    # -- dense ----------------------------------------------------------------------------------
    def gemm(self, A, B, Cm, a_k=True, b_k=True, alpha=1.0, beta=0.0, bias=None, splitk=1, lean=False, nt_x6=True):
        M, N, K, pa, lda, pb, ldb, pc, ldc, pbias, flags, ws, wsb = self._gemm_args(A, B, Cm, a_k, b_k, bias, splitk, lean, nt_x6)
        _lib.check(self.lib.fn_gemm_f32(int(a_k), int(b_k), M, N, K, alpha, pa, lda, pb, ldb, beta, pc, ldc, pbias, flags, ws, wsb, self.stream()),
                   "fn_gemm_f32")

    def gemm_plan(self, A, B, Cm, a_k=True, b_k=True, bias=None, splitk=1, lean=False, nt_x6=True):
        """what gemm() with these arguments launches, as the library decides it (fn_gemm_plan on the same prepared arguments, the workspace included):
        dict(kernel, klen, ranges, grid=(x, y, z), tiles, reduce, reduce_blocks, msplit).  Nothing is enqueued."""
        M, N, K, pa, lda, pb, ldb, pc, ldc, pbias, flags, ws, _ = self._gemm_args(A, B, Cm, a_k, b_k, bias, splitk, lean, nt_x6)
        plan = _lib.FnGemmPlan()
        _lib.check(self.lib.fn_gemm_plan(int(a_k), int(b_k), M, N, K, lda, ldb, ldc, pa, pb, pc, pbias, ws, flags, 0, C.byref(plan)), "fn_gemm_plan")
        return plan.as_dict()

    def _gemm_args(self, A, B, Cm, a_k, b_k, bias, splitk, lean, nt_x6):
        """the arguments of fn_gemm_f32 / fn_gemm_plan for one product: (M, N, K, A, lda, B, ldb, C, ldc, bias, splitk | flags, workspace, its bytes)"""
        pa, ar, ac, lda = _mat(A, "A")
        pb, br, bc, ldb = _mat(B, "B")
        pc, M, N, ldc = _mat(Cm, "C")
        K = ac if a_k else ar
        if (ar if a_k else ac) != M or (br if b_k else bc) != N or (bc if b_k else br) != K:
            raise RuntimeError("gemm shape mismatch A%s B%s C%s a_k=%s b_k=%s" % (tuple(A.shape), tuple(B.shape), tuple(Cm.shape), a_k, b_k))
        _chk(bias, name="bias")
        ws, wsb = None, 0
        x6 = _lib.GEMM_BF16X6 if (self.dw_x6 and not a_k and not b_k and K >= 1024) else 0
        if x6:
            splitk, x6 = self._x6_mode(splitk, N, K, x6)
        elif self.dw_x6 and self.nt_x6 and nt_x6 and a_k and b_k and splitk <= 1 and M % 128 == 0 and N % 128 == 0 and K % 32 == 0 and K >= 128 and (M // 128) * (N // 128) >= 128:
            x6 = _lib.GEMM_BF16X6                  # Linear forward / dX of the decoder pipeline on the bf16 MFMA (gemm_nt_x6w_kernel; the lean instance is then moot)
            if self.x6_per_tile:                   # (A/B, tests: one workgroup per tile instead of one per CU walking its tiles)
                x6 |= _lib.GEMM_X6_PERTILE
        if splitk > 1:
            wsb = self.lib.fn_gemm_ws_bytes(M, N, splitk & 0xffff)
            ws = self.workspace(wsb, "gemm")
        return M, N, K, pa, lda, pb, ldb, pc, ldc, _p(bias), splitk | (_lib.GEMM_LEAN if lean else 0) | x6, _p(ws), wsb

    def _x6_mode(self, splitk, N, K, x6):
        """kernel choice of a bf16 x 6 weight-gradient product: (K ranges, flags).  Wide (128 x 256) tiles halve the number of output tiles: twice the K
        ranges keep the number of workgroups (whole 32-k blocks per range permitting).  The per-wave kernel (tests, A/B) runs on the same K ranges."""
        if self.x6_wide == "force":                       # tests: the wide kernel on whatever shape and split, K ranges as given
            if not self.x6_perwave:
                x6 |= _lib.GEMM_X6_WIDE
        elif self.x6_wide and N >= 256 and splitk > 1 and K >= 32768:      # (K = 16384, the attribute decoders: 162 us on 128 x 128 tiles / 16 ranges, 172 on wide / 32)
            splitk *= 2
            if not self.x6_perwave:
                x6 |= _lib.GEMM_X6_WIDE
        if self.x6_perwave:
            x6 |= _lib.GEMM_X6_PERWAVE
        if self.x6_per_tile:
            x6 |= _lib.GEMM_X6_PERTILE
        return splitk, x6

    def gemm_multi(self, jobs, a_k=True, b_k=True):
        """jobs: dicts(C=2-D view, segs=[(A, B), ...] (<= 4 products summed), beta=0.0, bias=None) - independent GEMMs of one
        (a_k, b_k) form in ONE launch (fn_gemm_multi); more than 12 jobs are split into several launches"""
        for i0 in range(0, len(jobs), 12):
            part = jobs[i0:i0 + 12]
            arr = (_lib.FnGemmJob * len(part))()
            for d, j in zip(arr, part):
                pc, M, N, ldc = _mat(j["C"], "C")
                _chk(j.get("bias"), name="bias")
                d.M, d.N, d.C, d.ldc, d.bias, d.beta, d.n_seg = M, N, pc, ldc, _p(j.get("bias")), float(j.get("beta", 0.0)), len(j["segs"])
                if not 1 <= len(j["segs"]) <= 4:
                    raise RuntimeError("gemm_multi: 1..4 products per job")
                for sg, (A, B) in zip(d.seg, j["segs"]):
                    pa, ar, ac, lda = _mat(A, "A")
                    pb, br, bc, ldb = _mat(B, "B")
                    K = ac if a_k else ar
                    if (ar if a_k else ac) != M or (br if b_k else bc) != N or (bc if b_k else br) != K:
                        raise RuntimeError("gemm_multi shape mismatch A%s B%s C%s" % (tuple(A.shape), tuple(B.shape), (M, N)))
                    sg.A, sg.lda, sg.B, sg.ldb, sg.K = pa, lda, pb, ldb, K
            _lib.check(self.lib.fn_gemm_multi(int(a_k), int(b_k), arr, len(part), self.stream()), "fn_gemm_multi")

    def transpose(self, src, dst):
        ps, R, Cc, sld = _mat(src, "src")
        pd, dr, dc, dld = _mat(dst, "dst")
        if (dr, dc) != (Cc, R):
            raise RuntimeError("transpose shape mismatch %s -> %s" % (tuple(src.shape), tuple(dst.shape)))
        _lib.check(self.lib.fn_transpose_f32(ps, R, Cc, sld, pd, dld, self.stream()), "fn_transpose_f32")

    def colsum(self, X, out, beta=0.0):
        px, M, N, ld = _mat(X, "X")
        _dense(out, name="out")
        if out.numel() != N:
            raise RuntimeError("colsum: out has %d elements, expected %d" % (out.numel(), N))
        wsb = self.lib.fn_colsum_ws_bytes(M, N)
        ws = self.workspace(wsb, "colsum")
        _lib.check(self.lib.fn_colsum_f32(px, M, N, ld, beta, _p(out), _p(ws), wsb, self.stream()), "fn_colsum_f32")

    def colsum_multi(self, jobs):
        """jobs: (X 2-D view, out 1-D dense[, beta]) - all column sums in ONE launch per 64 jobs (fn_colsum_multi); meant for the
        bias gradients of a step (<= a few thousand rows each)"""
        for i0 in range(0, len(jobs), _lib.FN_COLSUM_MAX_JOBS):
            part = jobs[i0:i0 + _lib.FN_COLSUM_MAX_JOBS]
            arr = (_lib.FnColsumJob * len(part))()
            for d, j in zip(arr, part):
                X, out = j[0], j[1]
                px, M, N, ld = _mat(X, "X")
                _dense(out, name="out")
                if out.numel() != N:
                    raise RuntimeError("colsum_multi: out has %d elements, expected %d" % (out.numel(), N))
                d.X, d.M, d.N, d.ld, d.beta, d.out = px, M, N, ld, float(j[2]) if len(j) > 2 else 0.0, _p(out)
            _lib.check(self.lib.fn_colsum_multi(arr, len(part), self.stream()), "fn_colsum_multi")

    def occupy_cus(self, blocks, lds_bytes, cycles):
        """diagnostic (fn_occupy_cus): `blocks` workgroups holding `lds_bytes` of LDS each spin for ~`cycles` ticks on the current stream"""
        _lib.check(self.lib.fn_occupy_cus(int(blocks), int(lds_bytes), int(cycles), self.stream()), "fn_occupy_cus")

    def axpy(self, alpha, x, y):
        _dense(x, name="x"), _dense(y, name="y")
        if x.numel() != y.numel():
            raise RuntimeError("axpy size mismatch")
        _lib.check(self.lib.fn_axpy_f32(x.numel(), alpha, _p(x), _p(y), self.stream()), "fn_axpy_f32")

    def sum(self, x, out, scale=1.0):
        _dense(x, name="x"), _chk(out, name="out")
        _lib.check(self.lib.fn_sum_f32(_p(x), x.numel(), scale, _p(out), self.stream()), "fn_sum_f32")

    # -- GRU scans ------------------------------------------------------------------------------
    def gates_floats(self, B, H):
        """floats per time step of the (opaque, blocked) saved-gates buffer."""
        return int(self.lib.fn_gru_gates_floats(B, H))

    def frag_floats(self, rows, K):
        return int(self.lib.fn_frag_floats(rows, K))

    def frag_pack(self, src, dst):
        """row-major 2-D view -> fragment-major operand image (dst: 1-D buffer of frag_floats(rows, K))."""
        ps, rows, K, ld = _mat(src, "src")
        _dense(dst, name="dst")
        if dst.numel() < self.frag_floats(rows, K):
            raise RuntimeError("frag_pack: dst too small")
        _lib.check(self.lib.fn_frag_pack(ps, rows, K, ld, _p(dst), self.stream()), "fn_frag_pack")

    def weight_images(self, jobs):
        """jobs: (kind, src 2-D view, dst) with kind "transpose" (dst [C][R] contiguous), "frag" (fragment-major image of src), "frag_t"
        (fragment-major image of src^T), "frag3" / "frag3_t" (the same two as bf16 triple images), "copy" (dst [R][C] dense: an aligned image of a
        column slice) - all in ONE launch (fn_weight_images)"""
        kinds = {"transpose": 0, "frag": 1, "frag_t": 2, "frag3": 3, "frag3_t": 4, "copy": 5}
        for i0 in range(0, len(jobs), 56):
            part = jobs[i0:i0 + 56]
            arr = (_lib.FnWeightImage * len(part))()
            for d, (kind, src, dst) in zip(arr, part):
                ps, R, Cc, ld = _mat(src, "src")
                _dense(dst, name="dst")
                need = {"transpose": lambda: R * Cc, "copy": lambda: R * Cc, "frag": lambda: self.frag_floats(R, Cc), "frag_t": lambda: self.frag_floats(Cc, R),
                        "frag3": lambda: self.frag_floats(R, Cc) * 3 // 2, "frag3_t": lambda: self.frag_floats(Cc, R) * 3 // 2}[kind]()
                if dst.numel() < need:
                    raise RuntimeError("weight_images: dst too small for %s of %s" % (kind, tuple(src.shape)))
                d.src, d.dst, d.rows, d.cols, d.ld, d.kind = ps, _p(dst), R, Cc, ld, kinds[kind]
            _lib.check(self.lib.fn_weight_images(arr, len(part), self.stream()), "fn_weight_images")

    def _frag_ws(self, tag, i, n):
        return self.workspace(4 * n, "%s%d" % (tag, i))[:n]

    SYNC_REGIONS = 64

    def begin_capture(self):
        """call right before a hipGraph capture starts: the captured launches take counter regions 0, 1, ... of a pool whose
        zero-fill is the first node of the graph (see _sync_region)"""
        for ent in self.__dict__.get("_sync_pools", {}).values():
            ent["next"] = 0

    def _sync_region(self):
        """(counters of this launch, sticky error word, flag bits).  Arrival counters must be zero at launch.
        Eager launches: one private region per lane, zero-filled by the library in front of every launch (a memset node each).
        Captured launches (the training step replays ~50 weight-stationary launches): every lane owns a POOL of regions, each launch
        takes the next one, and ONE fill node zero-fills the whole pool at the start of the graph and whenever the rotation wraps -
        every replay therefore finds its regions zero, whatever ran in between."""
        words = int(self.lib.fn_gru_sync_ws_bytes()) // 4
        syncs = self.__dict__.setdefault("_syncs", {})
        if self.lane + "err" not in syncs:
            syncs[self.lane + "err"] = torch.zeros(32, dtype=torch.int32, device=self.device)
        err = syncs[self.lane + "err"]
        if not torch.cuda.is_current_stream_capturing():
            eager = self.__dict__.setdefault("_sync_eager", {})
            if self.lane not in eager:
                eager[self.lane] = torch.zeros(words, dtype=torch.int32, device=self.device)
            pools = self.__dict__.setdefault("_sync_pools", {})
            if self.lane not in pools:           # allocated here, outside of any capture
                pools[self.lane] = dict(pool=torch.zeros(self.SYNC_REGIONS, words, dtype=torch.int32, device=self.device), next=0)
            for ent in pools.values():
                ent["next"] = 0                  # whatever is captured next starts with the pool fill
            return eager[self.lane], err, 0
        pools = self.__dict__.setdefault("_sync_pools", {})
        ent = pools.get(self.lane)
        if ent is None:
            raise RuntimeError("weight-stationary launch captured before its lane ran once eagerly (the counter pool is allocated eagerly)")
        if ent["next"] == 0:
            ent["pool"].zero_()
        region = ent["pool"][ent["next"]]
        ent["next"] = (ent["next"] + 1) % self.SYNC_REGIONS
        return region, err, _lib.GRU_SYNC_ZEROED

    def gru_sync_error(self, clear=False):
        """True when a weight-stationary launch (scan or single-launch decode) gave up waiting: ONE D2H copy of all the sticky
        error words (host sync).  clear=True also resets them so that the caller can retry on the per-step kernels."""
        syncs = list(self.__dict__.get("_syncs", {}).values())
        if not syncs:
            return False
        words = torch.stack([t[-32] for t in syncs]).tolist()
        bad = any(int(w) != 0 for w in words)
        if bad and clear:
            for t in syncs:
                t[-32:].zero_()
        return bad

    def _fwd_descriptors(self, scans, cu_budget=0):
        arr = (_lib.FnGruFwd * len(scans))()
        for i, (d, s) in enumerate(zip(arr, scans)):
            for k in ("w_hh_frag", "b_hh", "b_ih", "h0", "gx_dense", "gx_table", "gx_rowbias", "h_all", "gates", "h0_frag", "h_last_frag"):
                _dense(s.get(k), name=k)
            for k in ("h0_frag", "h_last_frag"):       # (the size the launch's arithmetic needs is checked in gru_seq_fwd, once x6 is decided)
                if s.get(k) is not None and s[k].numel() * s[k].element_size() < self.frag_floats(s["B"], s["H"]) * 4:
                    raise RuntimeError("%s needs frag_floats(B, H) floats" % k)
            d.cu_budget = int(cu_budget)
            _dense(s.get("idx"), torch.int32, "idx")
            d.B, d.T, d.H, d.reverse = s["B"], s["T"], s["H"], int(s.get("reverse", 0))
            d.w_hh_frag, d.b_hh, d.b_ih, d.h0 = _p(s["w_hh_frag"]), _p(s["b_hh"]), _p(s.get("b_ih")), _p(s.get("h0"))
            d.gx_dense, d.gx_table, d.idx = _p(s.get("gx_dense")), _p(s.get("gx_table")), _p(s.get("idx"))
            d.idx_ld = s["idx"].shape[1] if s.get("idx") is not None else 0
            d.idx_shift, d.start_token = int(s.get("idx_shift", 0)), int(s.get("start_token", 0))
            d.gx_rowbias, d.h_all, d.gates = _p(s.get("gx_rowbias")), _p(s["h_all"]), _p(s.get("gates"))
            d.h0_frag, d.h_last_frag = _p(s.get("h0_frag")), _p(s.get("h_last_frag"))
        return arr

    def gru_fwd_x6_ok(self, scans, cu_budget=0):
        """would gru_seq_fwd run this launch on the bf16 x 6 kernels (fn_gru_fwd_x6_ok)?  The caller of a CHAIN of launches (time chunks that hand
        their state over as operand images) asks for every launch first and runs the whole chain on one arithmetic."""
        if not (self.dw_x6 and all(s.get("w_hh_frag3") is not None for s in scans)):
            return False
        return bool(self.lib.fn_gru_fwd_x6_ok(self._fwd_descriptors(scans, cu_budget), len(scans)))

    def gru_seq_fwd(self, scans, persistent=True, cu_budget=0, variant=None, x6=None):
        """x6: None = this launch decides for itself (bf16 x 6 where eligible, refused when it is part of a hand-over chain: h0_frag /
        h_last_frag images depend on the arithmetic), True / False = the decision the caller made for the whole chain"""
        arr, x6 = self._fwd_args(scans, persistent, cu_budget, variant, x6)
        _lib.check(self.lib.fn_gru_seq_fwd(arr, len(scans), self.stream()), "fn_gru_seq_fwd (bf16 x 6)" if x6 else "fn_gru_seq_fwd")

    def gru_fwd_plan(self, scans, persistent=True, cu_budget=0, variant=None, x6=None):
        """what gru_seq_fwd() with these arguments launches, as the library decides it on the current device (fn_gru_fwd_plan on the same prepared
        descriptors: workspaces, counter region, variant bits and the bf16 x 6 decision): dict(status, chosen, cus, ws_absent, candidates = [dict(kernel,
        rows_per_group, groups, grid, lds_bytes, fits, ..), ..] in the order they are tried).  Nothing is enqueued."""
        arr, _ = self._fwd_args(scans, persistent, cu_budget, variant, x6)
        plan = _lib.FnGruPlan()
        _lib.check(self.lib.fn_gru_fwd_plan(arr, len(scans), 0, C.byref(plan)), "fn_gru_fwd_plan")
        return plan.as_dict()

    def _fwd_args(self, scans, persistent, cu_budget, variant, x6):
        """the descriptors of fn_gru_seq_fwd / fn_gru_fwd_plan for one launch and its arithmetic: (FnGruFwd array, x6)"""
        arr = self._fwd_descriptors(scans, cu_budget)
        variant = self.variant if variant is None else variant
        sync = self._sync_region() if persistent else None
        if x6 is None:
            x6 = persistent and self.gru_fwd_x6_ok(scans, cu_budget)
            if x6 is False and self.dw_x6 and any(s.get("h0_frag") is not None or s.get("h_last_frag") is not None for s in scans) \
                    and all(s.get("w_hh_frag3") is not None for s in scans):
                raise RuntimeError("gru_seq_fwd: a launch of a hand-over chain must be told the chain's arithmetic (x6=True / False)")
        if x6 and not persistent:
            raise RuntimeError("gru_seq_fwd: the bf16 x 6 scans are weight-stationary launches")
        for i, (d, s) in enumerate(zip(arr, scans)):
            if x6:                               # hand-over images of a bf16 x 6 launch are triples: 6 bytes per value (an fp32-sized buffer would be overrun)
                for k in ("h0_frag", "h_last_frag"):
                    if s.get(k) is not None and s[k].numel() * s[k].element_size() < self.frag_floats(s["B"], s["H"]) * 6:
                        raise RuntimeError("%s of a bf16 x 6 launch needs 3/2 * frag_floats(B, H) floats (bf16 triples)" % k)
            d.frag_ws = _p(self._frag_ws("fragf", i, 3 * self.frag_floats(s["B"], s["H"])))      # 2 slabs of fp32 fragments, or 2 of bf16 triples (x6)
            d.sync_ws, d.err_ws, d.variant = (_p(sync[0]), _p(sync[1]), int(variant) | sync[2]) if persistent else (None, None, int(variant))
            if x6:
                d.w_hh_frag, d.variant = _p(s["w_hh_frag3"]), d.variant | _lib.GRU_BF16X6
        return arr, x6

    def frag3_pack(self, src, dst):
        """bf16 triple image of src [rows][K] (fn_frag3_pack); dst: 3/2 * frag_floats(rows, K) floats"""
        ps, R, K, ld = _mat(src, "src")
        _dense(dst, name="dst")
        if dst.numel() * dst.element_size() < self.frag_floats(R, K) * 6:
            raise RuntimeError("frag3_pack: dst too small")
        _lib.check(self.lib.fn_frag3_pack(ps, R, K, ld, _p(dst), self.stream()), "fn_frag3_pack")

    def gru_cell(self, h_prev, w_hh, b_hh, h_out, x=None, w_ih=None, b_ih=None, gx_table=None, idx=None, start_token=0, gx_rowbias=None, variant=None,
                 idx_best=None, best_v=0):
        """one GRUCell step of a large batch (fn_gru_cell_f32): h_out [B][H] from h_prev [B][H], optional dense input x [B][K1] with the
        torch matrix w_ih [3H][K1], optional token rows gx_table [V][3H] picked by idx (a [B] int32 column view, e.g. tokens[:, i - 1];
        None = start_token; or idx_best: the [B] int64 packed argmax words out_argmax left for the previous token, packed with best_v
        columns) and per-row constants gx_rowbias [B][3H]; w_hh [3H][H] is the torch matrix itself"""
        c = self._cell_args(h_prev, w_hh, b_hh, h_out, x, w_ih, b_ih, gx_table, idx, start_token, gx_rowbias, variant, idx_best, best_v)
        _lib.check(self.lib.fn_gru_cell_f32(C.byref(c), self.stream()), "fn_gru_cell_f32")

    def gru_cell_plan(self, h_prev, w_hh, b_hh, h_out, x=None, w_ih=None, b_ih=None, gx_table=None, idx=None, start_token=0, gx_rowbias=None, variant=None,
                      idx_best=None, best_v=0):
        """what gru_cell() with these arguments launches (fn_gru_cell_plan on the same prepared descriptor): dict(family, template, has_tab, has_rb, kmax,
        grid, threads, lds_bytes, forced_honoured).  Nothing is enqueued."""
        c = self._cell_args(h_prev, w_hh, b_hh, h_out, x, w_ih, b_ih, gx_table, idx, start_token, gx_rowbias, variant, idx_best, best_v)
        plan = _lib.FnGruCellPlan()
        _lib.check(self.lib.fn_gru_cell_plan(C.byref(c), C.byref(plan)), "fn_gru_cell_plan")
        _lib.check(plan.status, "fn_gru_cell_plan")
        return plan.as_dict()

    def _cell_args(self, h_prev, w_hh, b_hh, h_out, x, w_ih, b_ih, gx_table, idx, start_token, gx_rowbias, variant, idx_best, best_v):
        """the descriptor of fn_gru_cell_f32 / fn_gru_cell_plan"""
        c = _lib.FnGruCell()
        ph, B, H, ldh = _mat(h_prev, "h_prev")
        pw, r3, Hw, ldw = _mat(w_hh, "w_hh")
        po, Bo, Ho, ldo = _mat(h_out, "h_out")
        if r3 != 3 * H or Hw != H or (Bo, Ho) != (B, H):
            raise RuntimeError("gru_cell shape mismatch h_prev%s w_hh%s h_out%s" % (tuple(h_prev.shape), tuple(w_hh.shape), tuple(h_out.shape)))
        _dense(b_hh, name="b_hh"), _dense(b_ih, name="b_ih"), _dense(gx_table, name="gx_table"), _dense(gx_rowbias, name="gx_rowbias")
        c.B, c.H, c.h_prev, c.ldh, c.w_hh, c.ldw_hh, c.b_hh, c.b_ih, c.h_out, c.ldo = B, H, ph, ldh, pw, ldw, _p(b_hh), _p(b_ih), po, ldo
        if x is not None:
            px, Bx, K1, ldx = _mat(x, "x")
            pwi, r3i, K1w, ldwi = _mat(w_ih, "w_ih")
            if Bx != B or r3i != 3 * H or K1w != K1:
                raise RuntimeError("gru_cell: x%s / w_ih%s do not match" % (tuple(x.shape), tuple(w_ih.shape)))
            c.x, c.ldx, c.K1, c.w_ih, c.ldw_ih = px, ldx, K1, pwi, ldwi
        c.gx_table, c.gx_rowbias, c.start_token = _p(gx_table), _p(gx_rowbias), int(start_token)
        c.variant = int(self.cell_variant if variant is None else variant)
        if self.dw_x6 and self.cell_x6 and variant is None and B >= self.cell_x6_rows:
            # FnGruCell.variant | FN_GRU_BF16X6: the cell on the bf16 MFMA with exact triple splits where the shape allows it (B % 128 == 0, H % 32 == 0, K1 % 32 == 0), else
            # the fp32 cells.  Measured (scratch/r6_bench_decode_cells.py, us per token of the tokens-only decode): 2048 rows 90.0 against 95.7, 1536 rows 87.2
            # against 76.6, 1024 rows 87.2 against 59.5 - one 128-row workgroup per CU takes ~28 / 48 us for the 16 / 32 blocks of the two cells whatever the row
            # count, so it only pays where the fp32 cells need every CU: from 2048 rows on
            c.variant |= _lib.GRU_BF16X6
        if idx is not None:
            if idx.dtype != torch.int32 or idx.dim() != 1 or idx.shape[0] != B:
                raise RuntimeError("gru_cell: idx must be a [B] int32 column")
            c.idx, c.idx_ld = idx.data_ptr(), idx.stride(0)
        if idx_best is not None:
            if idx_best.dtype != torch.int64 or idx_best.dim() != 1 or idx_best.shape[0] != B or not idx_best.is_contiguous():
                raise RuntimeError("gru_cell: idx_best must be a contiguous [B] int64 row")
            c.idx_best, c.best_v = idx_best.data_ptr(), int(best_v)
        return c

    def out_argmax(self, h, W, bias, best):
        """fn_out_argmax_f32: best[b] = max(best[b], packed (logit, column) words of h[b] W^T + bias) - best: a ZEROED contiguous [B] int64 row"""
        _lib.check(self.lib.fn_out_argmax_f32(*self._out_argmax_args(h, W, bias, best), self.stream()), "fn_out_argmax_f32")

    def out_argmax_plan(self, h, W, bias, best):
        """what out_argmax() with these arguments launches (fn_out_argmax_plan on the same prepared arguments): dict(kernel, grid, threads, lds_bytes).
        Nothing is enqueued."""
        plan = _lib.FnOutArgmaxPlan()
        _lib.check(self.lib.fn_out_argmax_plan(*self._out_argmax_args(h, W, bias, best), C.byref(plan)), "fn_out_argmax_plan")
        _lib.check(plan.status, "fn_out_argmax_plan")
        return plan.as_dict()

    def _out_argmax_args(self, h, W, bias, best):
        """the arguments of fn_out_argmax_f32 / fn_out_argmax_plan in front of the stream / the plan"""
        ph, B, K, ldh = _mat(h, "h")
        pw, V, Kw, ldw = _mat(W, "W")
        _dense(bias, name="bias")
        if Kw != K or bias.numel() != V or best.dtype != torch.int64 or best.dim() != 1 or best.shape[0] != B or not best.is_contiguous():
            raise RuntimeError("out_argmax shape mismatch h%s W%s best%s" % (tuple(h.shape), tuple(W.shape), tuple(best.shape)))
        return ph, ldh, pw, ldw, _p(bias), B, V, K, best.data_ptr()

    def best_tokens(self, best, V, tokens):
        """fn_best_tokens: best [steps][B] int64 packed words -> tokens [B][steps] int32 (row stride tokens.stride(0))"""
        if best.dtype != torch.int64 or best.dim() != 2 or not best.is_contiguous() or tokens.dtype != torch.int32 or tokens.dim() != 2:
            raise RuntimeError("best_tokens: best [steps][B] int64, tokens [B][>= steps] int32")
        steps, B = best.shape
        if tokens.shape[0] != B or tokens.shape[1] < steps or tokens.stride(1) != 1:
            raise RuntimeError("best_tokens: tokens%s does not take %d x %d words" % (tuple(tokens.shape), steps, B))
        _lib.check(self.lib.fn_best_tokens(best.data_ptr(), steps, B, int(V), tokens.data_ptr(), tokens.stride(0), self.stream()), "fn_best_tokens")

    def _bwd_descriptors(self, scans, cu_budget=0):
        arr = (_lib.FnGruBwd * len(scans))()
        for d, s in zip(arr, scans):
            for k in ("w_hh_t_frag", "h0", "h_all", "gates", "dh_last", "dh_ext", "dgx_all", "dghn_all", "dh0", "dgx_rowsum", "dghn_rowsum", "scratch"):
                _dense(s.get(k), name=k)
            d.cu_budget = int(cu_budget)
            d.B, d.T, d.H = s["B"], s["T"], s["H"]
            d.w_hh_t_frag, d.h0, d.h_all, d.gates = _p(s["w_hh_t_frag"]), _p(s.get("h0")), _p(s["h_all"]), _p(s["gates"])
            d.dh_last, d.dh_ext = _p(s.get("dh_last")), _p(s.get("dh_ext"))
            d.dgx_all, d.dghn_all, d.dh0 = _p(s["dgx_all"]), _p(s["dghn_all"]), _p(s.get("dh0"))
            d.dgx_rowsum, d.dghn_rowsum, d.scratch = _p(s.get("dgx_rowsum")), _p(s.get("dghn_rowsum")), _p(s["scratch"])
        return arr

    def gru_bwd_x6_ok(self, scans, cu_budget=0):
        """would gru_seq_bwd run this launch on the bf16 x 6 kernel (fn_gru_bwd_x6_ok)?"""
        if not (self.dw_x6 and self.bwd_x6 and all(s.get("w_hh_t_frag3") is not None for s in scans)):
            return False
        arr = self._bwd_descriptors(scans, cu_budget)
        arr[0].variant = int(self.variant)
        return bool(self.lib.fn_gru_bwd_x6_ok(arr, len(scans)))

    def gru_seq_bwd(self, scans, persistent=True, cu_budget=0, variant=None, x6=None):
        """x6: None = bf16 x 6 where the launch is eligible (a backward launch hands nothing but fp32 tensors to the next one: every launch decides for
        itself), True / False = forced"""
        arr, x6, auto = self._bwd_args(scans, persistent, cu_budget, variant, x6)
        rc = self.lib.fn_gru_seq_bwd(arr, len(scans), self.stream())
        if rc == _lib.FN_E_UNSUPPORTED and x6 and auto:
            # the shape predicate said yes, a launch-time check (alignment, occupancy) said no: nothing was launched, and a backward launch hands only
            # fp32 tensors on - the fp32 kernels take it (a FORCED x6=True still raises)
            x6 = self._bwd_fp32(arr, scans)
            rc = self.lib.fn_gru_seq_bwd(arr, len(scans), self.stream())
        _lib.check(rc, "fn_gru_seq_bwd (bf16 x 6)" if x6 else "fn_gru_seq_bwd")

    def gru_bwd_plan(self, scans, persistent=True, cu_budget=0, variant=None, x6=None):
        """what gru_seq_bwd() with these arguments launches (fn_gru_bwd_plan on the same prepared descriptors, the repeat on the fp32 kernels
        included), as gru_fwd_plan.  Nothing is enqueued."""
        arr, x6, auto = self._bwd_args(scans, persistent, cu_budget, variant, x6)
        plan = _lib.FnGruPlan()
        _lib.check(self.lib.fn_gru_bwd_plan(arr, len(scans), 0, C.byref(plan)), "fn_gru_bwd_plan")
        if plan.status == _lib.FN_E_UNSUPPORTED and x6 and auto:
            self._bwd_fp32(arr, scans)
            _lib.check(self.lib.fn_gru_bwd_plan(arr, len(scans), 0, C.byref(plan)), "fn_gru_bwd_plan")
        return plan.as_dict()

    def _bwd_fp32(self, arr, scans):
        """bf16 x 6 descriptors -> the fp32 kernels' (the weight image and the bit); returns the new x6 = False"""
        for d, s in zip(arr, scans):
            d.w_hh_t_frag, d.variant = _p(s["w_hh_t_frag"]), d.variant & ~_lib.GRU_BF16X6
        return False

    def _bwd_args(self, scans, persistent, cu_budget, variant, x6):
        """the descriptors of fn_gru_seq_bwd / fn_gru_bwd_plan for one launch: (FnGruBwd array, x6, was x6 this launch's own decision)"""
        arr = self._bwd_descriptors(scans, cu_budget)
        variant = self.variant if variant is None else variant
        sync = self._sync_region() if persistent else None
        auto = x6 is None
        if auto:
            x6 = persistent and self.gru_bwd_x6_ok(scans, cu_budget)
        for i, (d, s) in enumerate(zip(arr, scans)):
            d.frag_ws = _p(self._frag_ws("fragb", i, 3 * self.frag_floats(s["B"], 3 * s["H"])))      # 2 slabs of fp32 fragments, or 2 of bf16 triples (x6)
            d.sync_ws, d.err_ws, d.variant = (_p(sync[0]), _p(sync[1]), int(variant) | sync[2]) if persistent else (None, None, int(variant))
            if x6:
                d.w_hh_t_frag, d.variant = _p(s["w_hh_t_frag3"]), d.variant | _lib.GRU_BF16X6
        return arr, x6, auto

    def gru_dwhh(self, dgx, dghn, hprev, dW, beta=0.0, splitk=1, lean=False):
        """dW [3H][H] = beta*dW + [dgx[:, :2H] | dghn]^T hprev  (dgx [rows][3H], dghn / hprev [rows][H])."""
        rows, H, flags, ws, wsb = self._dwhh_args(dgx, dghn, hprev, dW, splitk, lean)
        _lib.check(self.lib.fn_gru_dwhh_f32(_p(dgx), _p(dghn), _p(hprev), rows, H, beta, _p(dW), flags, ws, wsb, self.stream()), "fn_gru_dwhh_f32")

    def gru_dwhh_plan(self, dgx, dghn, hprev, dW, splitk=1, lean=False):
        """what gru_dwhh() with these arguments launches (fn_gru_dwhh_plan on the same prepared arguments): dict(form = 'one-launch' | 'two-products',
        launches = [plan, ..] as gemm_plan gives them).  Nothing is enqueued."""
        rows, H, flags, ws, _ = self._dwhh_args(dgx, dghn, hprev, dW, splitk, lean)
        n, plans = C.c_int32(), (_lib.FnGemmPlan * 2)()
        _lib.check(self.lib.fn_gru_dwhh_plan(_p(dgx), _p(dghn), _p(hprev), _p(dW), ws, rows, H, flags, 0, C.byref(n), plans), "fn_gru_dwhh_plan")
        return dict(form="one-launch" if n.value == 1 else "two-products", launches=[plans[i].as_dict() for i in range(n.value)])

    def _dwhh_args(self, dgx, dghn, hprev, dW, splitk, lean):
        """the arguments of fn_gru_dwhh_f32 / fn_gru_dwhh_plan: (rows, H, splitk | flags, workspace, its bytes)"""
        for t, nm in ((dgx, "dgx"), (dghn, "dghn"), (hprev, "hprev"), (dW, "dW")):
            _dense(t, name=nm)
        rows, H = hprev.shape
        if tuple(dgx.shape) != (rows, 3 * H) or tuple(dghn.shape) != (rows, H) or tuple(dW.shape) != (3 * H, H):
            raise RuntimeError("gru_dwhh shape mismatch")
        x6 = _lib.GEMM_BF16X6 if (self.dw_x6 and rows >= 1024) else 0
        if x6:
            splitk, x6 = self._x6_mode(splitk, H, rows, x6)
        wsb = int(self.lib.fn_gru_dwhh_ws_bytes(H, splitk))
        ws = self.workspace(wsb, "gemm") if wsb else None
        return rows, H, splitk | (_lib.GEMM_LEAN if lean else 0) | x6, _p(ws), wsb

    def decode_greedy(self, B, steps, H, V, start_token, w_hh1_frag, b_hh1, b_ih1, table1, rowbias1, h0, w_ih2_frag, b_ih2, w_hh2_frag, b_hh2,
                      w_out_frag, b_out, tokens, logp=None, forced=None, force=None):
        """single-launch greedy decode of <= 2048 sequences (fn_decode_greedy); tokens int32 [B][>=steps], logp [B][steps][V] or None.
        forced int32 [B][>=steps] + force uint8 [steps] on the device: fn_decode_forced (forced[b][i] is fed after step i where force[i])"""
        d, f = self._decode_args(B, steps, H, V, start_token, w_hh1_frag, b_hh1, b_ih1, table1, rowbias1, h0, w_ih2_frag, b_ih2, w_hh2_frag, b_hh2,
                                 w_out_frag, b_out, tokens, logp, forced, force)
        if f is not None:
            rc, what = self.lib.fn_decode_forced(C.byref(d), C.byref(f), self.stream()), "fn_decode_forced"
        else:
            rc, what = self.lib.fn_decode_greedy(C.byref(d), self.stream()), "fn_decode_greedy"
        if rc == _lib.FN_E_UNSUPPORTED:            # not eligible on this device (needs one CU per role workgroup)
            return False
        _lib.check(rc, what)
        return True

    def decode_plan(self, B, steps, H, V, start_token, w_hh1_frag, b_hh1, b_ih1, table1, rowbias1, h0, w_ih2_frag, b_ih2, w_hh2_frag, b_hh2,
                    w_out_frag, b_out, tokens, logp=None, forced=None, force=None):
        """what decode_greedy() with these arguments launches (fn_decode_plan on the same prepared descriptors, this device's compute units):
        dict(forced, mt, block_rows, nblk, nvt, nslices, per_rep, nrep, grid, threads, lds_bytes, the workspace offsets), or None where decode_greedy
        returns False (not eligible on this device).  Nothing is enqueued."""
        d, f = self._decode_args(B, steps, H, V, start_token, w_hh1_frag, b_hh1, b_ih1, table1, rowbias1, h0, w_ih2_frag, b_ih2, w_hh2_frag, b_hh2,
                                 w_out_frag, b_out, tokens, logp, forced, force)
        plan = _lib.FnDecodePlan()
        _lib.check(self.lib.fn_decode_plan(C.byref(d), None if f is None else C.byref(f), 0, C.byref(plan)), "fn_decode_plan")
        if plan.status == _lib.FN_E_UNSUPPORTED:
            return None
        _lib.check(plan.status, "fn_decode_plan")
        return plan.as_dict()

    def _decode_args(self, B, steps, H, V, start_token, w_hh1_frag, b_hh1, b_ih1, table1, rowbias1, h0, w_ih2_frag, b_ih2, w_hh2_frag, b_hh2,
                     w_out_frag, b_out, tokens, logp, forced, force):
        """the descriptors of fn_decode_greedy / fn_decode_forced / fn_decode_plan: (FnDecode, FnDecodeForce or None)"""
        d = _lib.FnDecode()
        for t, nm in ((w_hh1_frag, "w_hh1_frag"), (b_hh1, "b_hh1"), (b_ih1, "b_ih1"), (table1, "table1"), (rowbias1, "rowbias1"), (h0, "h0"),
                      (w_ih2_frag, "w_ih2_frag"), (b_ih2, "b_ih2"), (w_hh2_frag, "w_hh2_frag"), (b_hh2, "b_hh2"), (w_out_frag, "w_out_frag"),
                      (b_out, "b_out"), (logp, "logp")):
            _dense(t, name=nm)
            setattr(d, nm, _p(t))
        _dense(tokens, torch.int32, "tokens")
        d.B, d.steps, d.H, d.V, d.start_token = B, steps, H, V, start_token
        d.tokens, d.tok_ld = _p(tokens), tokens.shape[1]
        wsb = int(self.lib.fn_decode_ws_bytes(B, H, V))
        d.ws = _p(self.workspace(wsb, "decode"))
        syncs = self.__dict__.setdefault("_syncs", {})
        key = self.lane + "decode"
        if key not in syncs:
            syncs[key] = torch.zeros(int(self.lib.fn_decode_sync_ws_bytes()) // 4, dtype=torch.int32, device=self.device)
        d.sync_ws = _p(syncs[key])
        if forced is None and force is None:
            return d, None
        if forced is None or force is None:
            raise RuntimeError("decode_greedy: forced and force go together")
        _dense(forced, torch.int32, "forced"), _dense(force, torch.uint8, "force")
        if forced.shape[0] != B or forced.shape[1] < steps or force.numel() < steps:
            raise RuntimeError("decode_greedy: forced [B][>=steps] and force [steps] expected")
        f = _lib.FnDecodeForce()
        f.forced, f.forced_ld, f.force = _p(forced), forced.shape[1], _p(force)
        return d, f

    def embed_grad(self, dgx_all, idx, idx_shift, start_token, reverse, V, out):
        _dense(dgx_all, name="dgx_all"), _dense(idx, torch.int32, "idx"), _dense(out, name="out")
        T, B, N3 = dgx_all.shape
        wsb = self.lib.fn_embed_grad_ws_bytes(T * B, V, N3)
        ws = self.workspace(wsb, "embed")
        _lib.check(self.lib.fn_embed_grad_f32(_p(dgx_all), B, T, N3, _p(idx), idx.shape[1], idx_shift, start_token, int(reverse), V,
                                              _p(out), _p(ws), wsb, self.stream()), "fn_embed_grad_f32")

    def token_sort(self, idx, V, img=None):
        """counting sort of the (time, batch) positions of idx [B][T] by token -> handle for embed_grad_sorted.  ONE sort serves
        every scan that reads this token matrix (encoder directions, decoder layer 1)."""
        _dense(idx, torch.int32, "idx")
        B, T = idx.shape
        n = int(self.lib.fn_token_sort_ints(B * T, V))
        if img is None:
            img = torch.empty(n, dtype=torch.int32, device=self.device)
        _dense(img, torch.int32, "img")
        if img.numel() < n:
            raise RuntimeError("token_sort: img too small")
        wsb = int(self.lib.fn_token_sort_ws_bytes(B * T, V))
        ws = self.workspace(wsb, "toksort")
        _lib.check(self.lib.fn_token_sort(_p(idx), B, T, idx.shape[1], V, _p(img), _p(ws), wsb, self.stream()), "fn_token_sort")
        return dict(img=img, B=B, T=T, V=V)

    def embed_grad_sorted(self, handle, jobs):
        """jobs: dicts(dgx [T][B][N3], out = [V][N3] table view, or with transposed=True the [N3][V] view (e.g. dW_ih[:, :V]),
        reverse, idx_shift, start_token) - all reading the token matrix behind `handle`; one launch pair for all jobs."""
        B, T, V = handle["B"], handle["T"], handle["V"]
        arr = (_lib.FnEmbedGrad * len(jobs))()
        N3 = jobs[0]["dgx"].shape[2]
        for d, j in zip(arr, jobs):
            _dense(j["dgx"], name="dgx")
            if tuple(j["dgx"].shape) != (T, B, N3):
                raise RuntimeError("embed_grad_sorted: dgx must be [T][B][N3] of the sorted token matrix")
            po, r, c, ld = _mat(j["out"], "out")
            tr = bool(j.get("transposed", False))
            if (r, c) != ((N3, V) if tr else (V, N3)):
                raise RuntimeError("embed_grad_sorted: out has shape %s" % ((r, c),))
            d.dgx_all, d.out, d.out_ld, d.transposed = _p(j["dgx"]), po, ld, int(tr)
            d.reverse, d.idx_shift, d.start_token = int(j.get("reverse", 0)), int(j.get("idx_shift", 0)), int(j.get("start_token", 0))
        wsb = int(self.lib.fn_embed_grad_sorted_ws_bytes(B * T, B, V, N3, len(jobs)))
        ws = self.workspace(wsb, "embed")
        _lib.check(self.lib.fn_embed_grad_sorted(arr, len(jobs), B, T, N3, V, _p(handle["img"]), _p(ws), wsb, self.stream()), "fn_embed_grad_sorted")

    def time_sum(self, X, out):
        """out[...] = sum over the leading (time) axis of X."""
        _dense(X, name="X"), _dense(out, name="out")
        T = X.shape[0]
        M = X.numel() // T
        if out.numel() != M:
            raise RuntimeError("time_sum: out has %d elements, expected %d" % (out.numel(), M))
        _lib.check(self.lib.fn_time_sum_f32(_p(X), T, M, _p(out), self.stream()), "fn_time_sum_f32")

    # -- heads ----------------------------------------------------------------------------------
    def vocab_logsoftmax(self, logits, B, T, E, logp_bt=None, target=None, nll_rows=None, grad_scale=0.0, dlogits=None):
        pl, rows, _, ld = _mat(logits, "logits")
        _dense(logp_bt, name="logp_bt"), _dense(target, torch.int32, "target"), _dense(nll_rows, name="nll_rows")
        if dlogits is not None and _mat(dlogits, "dlogits")[3] != ld:
            raise RuntimeError("dlogits must share the leading dimension of logits")
        _lib.check(self.lib.fn_vocab_logsoftmax(pl, B, T, E, ld, _p(logp_bt), _p(target), _p(nll_rows), grad_scale, _p(dlogits),
                                                self.stream()), "fn_vocab_logsoftmax")

    def out_head(self, h, W, bias, B, T, target, nll_rows=None, grad_scale=0.0, dlogits=None):
        """fused output head (fn_out_head_f32): h [T*B][H] time-major rows, W [V][H], bias [V], target [B][T] int32 ->
        nll_rows [T*B] and / or dlogits [T*B][ld] = grad_scale * (softmax(h W^T + b) - onehot); the logits are not materialised"""
        ph, R, H, ldh = _mat(h, "h")
        pw, V, Hw, ldw = _mat(W, "W")
        if R != B * T or Hw != H:
            raise RuntimeError("out_head shape mismatch h%s W%s B=%d T=%d" % (tuple(h.shape), tuple(W.shape), B, T))
        _dense(bias, name="bias"), _dense(target, torch.int32, "target"), _dense(nll_rows, name="nll_rows")
        pd, ld = None, 0
        if dlogits is not None:
            pd, rows, _, ld = _mat(dlogits, "dlogits")
            if rows != R:
                raise RuntimeError("out_head: dlogits has %d rows, expected %d" % (rows, R))
        _lib.check(self.lib.fn_out_head_f32(ph, ldh, pw, ldw, _p(bias), B, T, V, H, _p(target), grad_scale, _p(nll_rows), pd, ld,
                                            self.stream()), "fn_out_head_f32")

    def vocab_logsoftmax_bwd(self, logp_bt, gout_bt, dlogits):
        _dense(logp_bt, name="logp_bt"), _dense(gout_bt, name="gout_bt")
        B, T, E = logp_bt.shape
        pd, _, _, ld = _mat(dlogits, "dlogits")
        _lib.check(self.lib.fn_vocab_logsoftmax_bwd(_p(logp_bt), _p(gout_bt), B, T, E, ld, pd, self.stream()), "fn_vocab_logsoftmax_bwd")

    def vocab_argmax(self, logits, E, logp_out, tok_out):
        """logits [B][ld]; logp_out: 2-D view [B][E] (any row stride) or None; tok_out: int32 1-D view (any stride)."""
        pl, B, _, ld = _mat(logits, "logits")
        _chk(tok_out, torch.int32, "tok_out")
        lp_ld = 0
        if logp_out is not None:
            _chk(logp_out, name="logp_out")
            lp_ld = logp_out.stride(0)
        _lib.check(self.lib.fn_vocab_argmax(pl, B, E, ld, _p(logp_out), lp_ld, _p(tok_out), tok_out.stride(0) if tok_out.dim() else 1,
                                            self.stream()), "fn_vocab_argmax")

    def vocab_sample(self, logits, E, params, step, logp_out, tok_out, own_out=None, u_out=None):
        """fn_vocab_sample: logits [B][ld]; params: the 32 bytes of FnSampleParams on the device; logp_out: 2-D view [B][E] (any row stride) or None;
        tok_out (the drawn tokens) / own_out (the first-index argmax, or None): int32 1-D views (any stride); u_out: [B] floats or None."""
        pl, B, _, ld = _mat(logits, "logits")
        _chk(tok_out, torch.int32, "tok_out"), _chk(own_out, torch.int32, "own_out")
        _dense(params, torch.uint8, "params"), _dense(u_out, name="u_out")
        if params.numel() != C.sizeof(_lib.FnSampleParams) or (u_out is not None and u_out.numel() < B):
            raise RuntimeError("vocab_sample: params holds %d bytes, FnSampleParams %d; u_out one float per row" % (params.numel(), C.sizeof(_lib.FnSampleParams)))
        lp_ld = 0
        if logp_out is not None:
            _chk(logp_out, name="logp_out")
            lp_ld = logp_out.stride(0)
        _lib.check(self.lib.fn_vocab_sample(pl, B, E, ld, _p(params), step, _p(logp_out), lp_ld, _p(own_out),
                                            0 if own_out is None else (own_out.stride(0) if own_out.dim() else 1), _p(tok_out),
                                            tok_out.stride(0) if tok_out.dim() else 1, _p(u_out), self.stream()), "fn_vocab_sample")

    def beam_step(self, logits, W, V, step, eos, score_prev, token_prev, score, parent, token, logp_out=None):
        """fn_beam_step: logits [B*W][ld]; score_prev / token_prev (None at step 0) and score / parent / token: 2-D views [B][W] (fp32 / int32, any row
        stride, the two previous ones sharing theirs, the three outputs theirs); eos: a token or -1; logp_out: 2-D view [B*W][V] (any row stride) or None"""
        pl, rows, _, ld = _mat(logits, "logits")
        if rows % W or any(t is not None and (t.dim() != 2 or tuple(t.shape) != (rows // W, W) or (W > 1 and t.stride(1) != 1))
                           for t in (score_prev, token_prev, score, parent, token)):
            raise RuntimeError("beam_step: %d rows do not make [B][%d] slabs" % (rows, W))
        _chk(score_prev, name="score_prev"), _chk(token_prev, torch.int32, "token_prev"), _chk(score, name="score")
        _chk(parent, torch.int32, "parent"), _chk(token, torch.int32, "token")
        sld = lambda t: t.stride(0) if t.shape[0] > 1 else max(W, t.stride(0))      # noqa: E731
        if len({sld(t) for t in (score, parent, token)}) != 1 or (score_prev is not None and token_prev is not None and sld(score_prev) != sld(token_prev)):
            raise RuntimeError("beam_step: the slabs of one step share a row stride")
        lp_ld = 0
        if logp_out is not None:
            _chk(logp_out, name="logp_out")
            lp_ld = logp_out.stride(0)
        _lib.check(self.lib.fn_beam_step(pl, rows // W, W, V, ld, int(step), int(eos), _p(score_prev), _p(token_prev),
                                         0 if score_prev is None else sld(score_prev), _p(score), _p(parent), _p(token), sld(score), _p(logp_out), lp_ld,
                                         self.stream()), "fn_beam_step")

    def beam_gather(self, jobs, parent, W):
        """fn_beam_gather: jobs = up to 4 (src, dst) pairs of 2-D views [rows][cols]; dst[r] = src[(r // W) * W + parent[r]]; parent: contiguous [rows] int32"""
        arr = (_lib.FnBeamGatherJob * len(jobs))()
        _dense(parent, torch.int32, "parent")
        rows = parent.numel()
        for j, (src, dst) in zip(arr, jobs):
            ps, rs, cs, lds = _mat(src, "src")
            pd, rd, cd, ldd = _mat(dst, "dst")
            if (rs, cs) != (rd, cd) or rs != rows:
                raise RuntimeError("beam_gather: src%s dst%s for %d rows" % (tuple(src.shape), tuple(dst.shape), rows))
            j.src, j.src_ld, j.dst, j.dst_ld, j.cols = ps, lds, pd, ldd, cs
        _lib.check(self.lib.fn_beam_gather(arr, len(jobs), rows, int(W), _p(parent), self.stream()), "fn_beam_gather")

    def beam_backtrack(self, parent, token, score, eos, tokens_out, len_out, score_out, beam_out=None, cum_out=None):
        """fn_beam_backtrack: contiguous slabs [steps][B][W] -> tokens_out / beam_out / cum_out [B][W][steps], len_out / score_out [B][W]"""
        steps, B, W = parent.shape
        for t, d, n, shp in ((parent, torch.int32, "parent", (steps, B, W)), (token, torch.int32, "token", (steps, B, W)), (score, torch.float32, "score", (steps, B, W)),
                             (tokens_out, torch.int32, "tokens_out", (B, W, steps)), (beam_out, torch.int32, "beam_out", (B, W, steps)),
                             (cum_out, torch.float32, "cum_out", (B, W, steps)), (len_out, torch.int32, "len_out", (B, W)), (score_out, torch.float32, "score_out", (B, W))):
            _dense(t, d, n)
            if t is not None and tuple(t.shape) != shp:
                raise RuntimeError("beam_backtrack: %s%s, expected %s" % (n, tuple(t.shape), shp))
        _lib.check(self.lib.fn_beam_backtrack(_p(parent), _p(token), _p(score), steps, B, W, int(eos), _p(tokens_out), _p(beam_out), _p(cum_out),
                                              _p(len_out), _p(score_out), self.stream()), "fn_beam_backtrack")

    def constrain_apply(self, logits, V, step, params, bias=None, held=None, stuck=None):
        """fn_constrain_apply, in place on logits [rows][ld]; params: the 32 bytes of FnConstrainParams on the device; bias: [V] (shared) or a 2-D view
        [rows][V] (any row stride), fp32, or None; held: contiguous [rows][4] int32 (the 128 sounding-pitch bits) or None; stuck: [rows] int32 or None"""
        pl, rows, _, ld = _mat(logits, "logits")
        _dense(params, torch.uint8, "params"), _dense(held, torch.int32, "held"), _dense(stuck, torch.int32, "stuck")
        bias_rs = 0
        if bias is not None and bias.dim() == 2:
            _, br, bc, bias_rs = _mat(bias, "bias")
        else:
            _dense(bias, name="bias")
            br, bc = rows, (V if bias is None else bias.numel())
        if (params.numel() != C.sizeof(_lib.FnConstrainParams) or (br, bc) != (rows, V) or (held is not None and tuple(held.shape) != (rows, 4))
                or (stuck is not None and stuck.numel() != rows)):
            raise RuntimeError("constrain_apply: params of %d bytes, bias / held / stuck for %d rows of %d tokens" % (C.sizeof(_lib.FnConstrainParams), rows, V))
        _lib.check(self.lib.fn_constrain_apply(pl, rows, V, ld, int(step), _p(params), _p(bias), bias_rs, _p(held), _p(stuck), self.stream()),
                   "fn_constrain_apply")

    def constrain_advance(self, tok, V, params, logits=None, fallback=None, held_in=None, held_out=None, fixed=None):
        """fn_constrain_advance: tok / fallback: int32 1-D views [rows] (any stride); logits [rows][ld] (then the fix-up runs and may rewrite tok) or None;
        held_in / held_out: contiguous [rows][4] int32 (may be the same tensor) or None; fixed: [rows] int32 or None"""
        _chk(tok, torch.int32, "tok"), _chk(fallback, torch.int32, "fallback")
        _dense(params, torch.uint8, "params"), _dense(held_in, torch.int32, "held_in"), _dense(held_out, torch.int32, "held_out"), _dense(fixed, torch.int32, "fixed")
        rows = tok.numel()
        pl, ld = None, 0
        if logits is not None:
            pl, lr, _, ld = _mat(logits, "logits")
            if lr != rows or fallback is None or fallback.numel() != rows:
                raise RuntimeError("constrain_advance: logits and fallback for %d rows" % rows)
        if (tok.dim() != 1 or params.numel() != C.sizeof(_lib.FnConstrainParams) or (held_in is None) != (held_out is None)
                or any(h is not None and tuple(h.shape) != (rows, 4) for h in (held_in, held_out)) or (fixed is not None and fixed.numel() != rows)):
            raise RuntimeError("constrain_advance: a 1-D tok, params of %d bytes, held_in and held_out [%d][4]" % (C.sizeof(_lib.FnConstrainParams), rows))
        _lib.check(self.lib.fn_constrain_advance(_p(tok), max(1, tok.stride(0)), rows, V, _p(params), pl, ld, _p(fallback),
                                                 1 if fallback is None else max(1, fallback.stride(0)), _p(held_in), _p(held_out), _p(fixed),
                                                 self.stream()), "fn_constrain_advance")

    def event_attributes(self, tokens, steps, params, n_cells, status, r_density, n_density, c_r, c_n, rhythm=None, notes=None, cells_ld=_lib.FN_ATTR_MAX_CELLS):
        """fn_event_attributes: tokens int32 [rows][>= steps] (any row stride); params: the 48 bytes of FnAttrParams on the device; six [rows] outputs;
        rhythm / notes: contiguous uint8 [rows][cells_ld] or None"""
        _chk(tokens, torch.int32, "tokens"), _dense(params, torch.uint8, "params")
        if tokens.dim() != 2 or (tokens.shape[1] > 1 and tokens.stride(1) != 1) or tokens.shape[1] < steps:
            raise RuntimeError("event_attributes: tokens 2-D with contiguous rows of at least %d, got shape %s strides %s" % (steps, tuple(tokens.shape), tokens.stride()))
        rows = tokens.shape[0]
        ld = tokens.stride(0) if rows > 1 else max(tokens.shape[1], tokens.stride(0))
        for t, d, nm in ((n_cells, torch.int32, "n_cells"), (status, torch.int32, "status"), (r_density, torch.float32, "r_density"),
                         (n_density, torch.float32, "n_density"), (c_r, torch.int32, "c_r"), (c_n, torch.int32, "c_n")):
            _dense(t, d, nm)
            if t is None or t.numel() != rows:
                raise RuntimeError("event_attributes: %s for %d rows" % (nm, rows))
        for t, nm in ((rhythm, "rhythm"), (notes, "notes")):
            _dense(t, torch.uint8, nm)
            if t is not None and tuple(t.shape) != (rows, cells_ld):
                raise RuntimeError("event_attributes: %s%s, expected %s" % (nm, tuple(t.shape), (rows, cells_ld)))
        if params.numel() != C.sizeof(_lib.FnAttrParams):
            raise RuntimeError("event_attributes: params of %d bytes" % C.sizeof(_lib.FnAttrParams))
        _lib.check(self.lib.fn_event_attributes(_p(tokens), ld, rows, int(steps), _p(params), _p(n_cells), _p(status), _p(r_density), _p(n_density), _p(c_r),
                                                _p(c_n), _p(rhythm), _p(notes), int(cells_ld), self.stream()), "fn_event_attributes")

    def notes_from_tokens(self, tokens, steps, params, notes, n_notes, t_end, status):
        """fn_notes_from_tokens: tokens int32 [rows][>= steps] (any row stride); params: the 64 bytes of FnNoteParams on the device; notes: contiguous
        int32 [rows][notes_ld][4]; three [rows] outputs"""
        _chk(tokens, torch.int32, "tokens"), _dense(params, torch.uint8, "params"), _dense(notes, torch.int32, "notes")
        if tokens.dim() != 2 or (tokens.shape[1] > 1 and tokens.stride(1) != 1) or tokens.shape[1] < steps:
            raise RuntimeError("notes_from_tokens: tokens 2-D with contiguous rows of at least %d, got shape %s strides %s" % (steps, tuple(tokens.shape), tokens.stride()))
        rows = tokens.shape[0]
        ld = tokens.stride(0) if rows > 1 else max(tokens.shape[1], tokens.stride(0))
        if notes.dim() != 3 or notes.shape[0] != rows or notes.shape[2] != 4:
            raise RuntimeError("notes_from_tokens: notes (%d, notes_ld, 4), got %s" % (rows, tuple(notes.shape)))
        for t, nm in ((n_notes, "n_notes"), (t_end, "t_end"), (status, "status")):
            _dense(t, torch.int32, nm)
            if t is None or t.numel() != rows:
                raise RuntimeError("notes_from_tokens: %s for %d rows" % (nm, rows))
        if params.numel() != C.sizeof(_lib.FnNoteParams):
            raise RuntimeError("notes_from_tokens: params of %d bytes" % C.sizeof(_lib.FnNoteParams))
        _lib.check(self.lib.fn_notes_from_tokens(_p(tokens), ld, rows, int(steps), _p(params), _p(notes), notes.shape[1], _p(n_notes), _p(t_end), _p(status),
                                                 self.stream()), "fn_notes_from_tokens")

    def tokens_from_notes(self, notes, spans, params, tokens, steps, n_tokens, n_kept, status):
        """fn_tokens_from_notes: notes contiguous int32 [n_total][4], spans contiguous int32 [rows][4]; params: the 64 bytes of FnNoteParams on the
        device; tokens int32 [rows][>= steps] (any row stride) and three [rows] outputs are written"""
        _dense(notes, torch.int32, "notes"), _dense(spans, torch.int32, "spans"), _dense(params, torch.uint8, "params"), _chk(tokens, torch.int32, "tokens")
        if notes.dim() != 2 or notes.shape[1] != 4 or spans.dim() != 2 or spans.shape[1] != 4:
            raise RuntimeError("tokens_from_notes: notes (n_total, 4) and spans (rows, 4), got %s and %s" % (tuple(notes.shape), tuple(spans.shape)))
        rows = spans.shape[0]
        if tokens.dim() != 2 or tokens.shape[0] != rows or (tokens.shape[1] > 1 and tokens.stride(1) != 1) or tokens.shape[1] < steps:
            raise RuntimeError("tokens_from_notes: tokens (%d, >= %d) with contiguous rows, got shape %s strides %s" % (rows, steps, tuple(tokens.shape), tokens.stride()))
        ld = tokens.stride(0) if rows > 1 else max(tokens.shape[1], tokens.stride(0))
        for t, nm in ((n_tokens, "n_tokens"), (n_kept, "n_kept"), (status, "status")):
            _dense(t, torch.int32, nm)
            if t is None or t.numel() != rows:
                raise RuntimeError("tokens_from_notes: %s for %d rows" % (nm, rows))
        if params.numel() != C.sizeof(_lib.FnNoteParams):
            raise RuntimeError("tokens_from_notes: params of %d bytes" % C.sizeof(_lib.FnNoteParams))
        _lib.check(self.lib.fn_tokens_from_notes(_p(notes) if notes.shape[0] else None, notes.shape[0], _p(spans), rows, _p(params), _p(tokens), ld, int(steps),
                                                 _p(n_tokens), _p(n_kept), _p(status), self.stream()), "fn_tokens_from_notes")

    def notes_stitch(self, dec, dec_ld, dec_n, dec_end, src, spans, mode, out, win_first, out_n, status):
        """fn_notes_stitch: dec int32 [S*V][>= dec_ld][4] (any row stride that is a multiple of 4 words; row = j*V + v), dec_n, dec_end, mode contiguous
        int32 [S*V]; src contiguous int32 [n_total][4], spans contiguous int32 [S][4]; out contiguous int32 [V][out_ld][4], win_first [V][S + 1], out_n and
        status [V] are written"""
        _chk(dec, torch.int32, "dec"), _dense(src, torch.int32, "src"), _dense(spans, torch.int32, "spans"), _dense(out, torch.int32, "out")
        if spans.dim() != 2 or spans.shape[1] != 4 or src.dim() != 2 or src.shape[1] != 4 or out.dim() != 3 or out.shape[2] != 4:
            raise RuntimeError("notes_stitch: spans (S, 4), src (n_total, 4) and out (V, out_ld, 4), got %s, %s and %s" % (
                tuple(spans.shape), tuple(src.shape), tuple(out.shape)))
        S, V = spans.shape[0], out.shape[0]
        rows = S * V
        if dec.dim() != 3 or dec.shape[0] != rows or dec.shape[2] != 4 or dec.shape[1] < dec_ld or dec.stride(2) != 1 or dec.stride(1) != 4 or (
                rows > 1 and (dec.stride(0) % 4 or dec.stride(0) < 4 * dec.shape[1])):
            raise RuntimeError("notes_stitch: dec (%d, >= %d, 4) with contiguous rows, got shape %s strides %s" % (rows, dec_ld, tuple(dec.shape), dec.stride()))
        rs = dec.stride(0) // 4 if rows > 1 else dec.shape[1]
        for t, nm, n in ((dec_n, "dec_n", rows), (dec_end, "dec_end", rows), (mode, "mode", rows), (win_first, "win_first", V * (S + 1)), (out_n, "out_n", V),
                         (status, "status", V)):
            _dense(t, torch.int32, nm)
            if t is None or t.numel() != n:
                raise RuntimeError("notes_stitch: %s of %d words" % (nm, n))
        _lib.check(self.lib.fn_notes_stitch(_p(dec), rs, int(dec_ld), _p(dec_n), _p(dec_end), _p(src) if src.shape[0] else None, src.shape[0], _p(spans), S, V,
                                            _p(mode), _p(out), out.shape[1], _p(win_first), _p(out_n), _p(status), self.stream()), "fn_notes_stitch")

    def latent_draw(self, jobs, params):
        """fn_latent_draw: jobs = up to 4 dicts of mu_lk, lv_lk (contiguous fp32 [K][Z]), z (a 2-D fp32 view [rows][Z] with unit inner stride; all jobs
        share its row stride), stream_id and optionally comp, comp_out (contiguous int32 [rows]) and eps_out (contiguous fp32 [rows][Z]); params: the
        32 bytes of FnDrawParams on the device"""
        _dense(params, torch.uint8, "params")
        if params.numel() != C.sizeof(_lib.FnDrawParams) or not 1 <= len(jobs) <= _lib.FN_DRAW_MAX_JOBS:
            raise RuntimeError("latent_draw: 1..%d jobs and %d parameter bytes, got %d and %d" % (
                _lib.FN_DRAW_MAX_JOBS, C.sizeof(_lib.FnDrawParams), len(jobs), params.numel()))
        arr = (_lib.FnDrawJob * len(jobs))()
        pz, rows, Z, z_ld = _mat(jobs[0]["z"], "z")
        for j, d in zip(arr, jobs):
            pz, r, zc, ld = _mat(d["z"], "z")
            mu, lv, comp, eps_out, comp_out = d["mu_lk"], d["lv_lk"], d.get("comp"), d.get("eps_out"), d.get("comp_out")
            _dense(mu, name="mu_lk"), _dense(lv, name="lv_lk"), _dense(comp, torch.int32, "comp"), _dense(eps_out, name="eps_out")
            _dense(comp_out, torch.int32, "comp_out")
            if (r, zc, ld) != (rows, Z, z_ld) or mu.dim() != 2 or mu.shape[1] != Z or lv.shape != mu.shape or any(
                    t is not None and t.numel() != n for t, n in ((comp, rows), (comp_out, rows), (eps_out, rows * Z))):
                raise RuntimeError("latent_draw: every job writes (%d, %d) at a row stride of %d from [K][%d] tables; comp, comp_out of %d, eps_out of %d "
                                   "entries" % (rows, Z, z_ld, Z, rows, rows * Z))
            j.mu_lk, j.lv_lk, j.comp, j.z, j.eps_out, j.comp_out, j.K, j.stream_id = (
                mu.data_ptr(), lv.data_ptr(), None if comp is None else comp.data_ptr(), d["z"].data_ptr(), None if eps_out is None else eps_out.data_ptr(),
                None if comp_out is None else comp_out.data_ptr(), mu.shape[0], int(d["stream_id"]))
        _lib.check(self.lib.fn_latent_draw(arr, len(jobs), rows, Z, z_ld, _p(params), self.stream()), "fn_latent_draw")

    def latent_mix(self, a, b, t, segs, out, omega_out=None, per_pair=False):
        """fn_latent_mix: a, b 2-D fp32 views [pairs][D] sharing a row stride; t contiguous fp32 [P], or [pairs][P] with per_pair; segs: up to 4
        (off, len, mode); out a 2-D fp32 view [pairs*P][D]; omega_out contiguous fp32 [pairs][len(segs)] or None"""
        pa, pairs, D, ld = _mat(a, "a")
        pb, rb, cb, ldb = _mat(b, "b")
        po, ro, co, ldo = _mat(out, "out")
        _dense(t, name="t"), _dense(omega_out, name="omega_out")
        P = t.numel() // pairs if per_pair else t.numel()
        if (rb, cb, ldb) != (pairs, D, ld) or P < 1 or t.numel() != (pairs * P if per_pair else P) or (ro, co) != (pairs * P, D) or not (
                1 <= len(segs) <= _lib.FN_MIX_MAX_SEGS) or (omega_out is not None and omega_out.numel() != pairs * len(segs)):
            raise RuntimeError("latent_mix: a%s b%s (strides %d, %d) t%s out%s for %d segments" % (
                tuple(a.shape), tuple(b.shape), ld, ldb, tuple(t.shape), tuple(out.shape), len(segs)))
        arr = (_lib.FnMixSeg * len(segs))()
        for s, (off, n, mode) in zip(arr, segs):
            s.off, s.len, s.mode, s.reserved = int(off), int(n), int(mode), 0
        _lib.check(self.lib.fn_latent_mix(pa, pb, ld, pairs, D, _p(t), P, 1 if per_pair else 0, arr, len(segs), po, ldo, _p(omega_out), self.stream()),
                   "fn_latent_mix")

    def posterior_draw(self, jobs, S, params):
        """fn_posterior_draw: jobs = up to 4 dicts of pre (contiguous fp32 [B][2Z]: mu | log sigma), mu_lk, lv_lk (contiguous fp32 [K][Z]), z (a 2-D fp32
        view [B*S][Z] with unit inner stride; all jobs share its row stride), logq, logp (contiguous fp64 [B*S]), stream_id and optionally eps_out
        (contiguous fp32 [B*S][Z]); params: the 32 bytes of FnDrawParams on the device"""
        _dense(params, torch.uint8, "params")
        if params.numel() != C.sizeof(_lib.FnDrawParams) or not 1 <= len(jobs) <= _lib.FN_DRAW_MAX_JOBS:
            raise RuntimeError("posterior_draw: 1..%d jobs and %d parameter bytes, got %d and %d" % (
                _lib.FN_DRAW_MAX_JOBS, C.sizeof(_lib.FnDrawParams), len(jobs), params.numel()))
        arr = (_lib.FnPostJob * len(jobs))()
        pz, rows, Z, z_ld = _mat(jobs[0]["z"], "z")
        S = int(S)
        B = rows // S if S > 0 else 0
        for j, d in zip(arr, jobs):
            pz, r, zc, ld = _mat(d["z"], "z")
            pre, mu, lv, eps_out, logq, logp = d["pre"], d["mu_lk"], d["lv_lk"], d.get("eps_out"), d["logq"], d["logp"]
            _dense(pre, name="pre"), _dense(mu, name="mu_lk"), _dense(lv, name="lv_lk"), _dense(eps_out, name="eps_out")
            _dense(logq, torch.float64, "logq"), _dense(logp, torch.float64, "logp")
            if B < 1 or B * S != rows or (r, zc, ld) != (rows, Z, z_ld) or tuple(pre.shape) != (B, 2 * Z) or mu.dim() != 2 or mu.shape[1] != Z or (
                    lv.shape != mu.shape) or logq.numel() != rows or logp.numel() != rows or (eps_out is not None and eps_out.numel() != rows * Z):
                raise RuntimeError("posterior_draw: every job writes (%d, %d) = (B*%d, Z) at a row stride of %d from pre (B, %d) and [K][%d] tables; logq, "
                                   "logp of %d, eps_out of %d entries" % (rows, Z, S, z_ld, 2 * Z, Z, rows, rows * Z))
            j.pre, j.mu_lk, j.lv_lk, j.z, j.eps_out, j.logq, j.logp, j.K, j.stream_id = (
                pre.data_ptr(), mu.data_ptr(), lv.data_ptr(), d["z"].data_ptr(), None if eps_out is None else eps_out.data_ptr(), logq.data_ptr(),
                logp.data_ptr(), mu.shape[0], int(d["stream_id"]))
        _lib.check(self.lib.fn_posterior_draw(arr, len(jobs), B, S, Z, z_ld, _p(params), self.stream()), "fn_posterior_draw")

    def iw_reduce(self, nll, B, S, logp, logq, lw, out, t0=None, t1=None):
        """fn_iw_reduce: nll a 2-D fp32 view [T][B*S] with unit inner stride (fn_out_head_f32's nll_rows); logp, logq 2-D fp64 views [n_lat][B*S] sharing a
        row stride; lw contiguous fp64 [B*S]; out a 2-D fp64 view [B][4 + n_lat]; t0, t1 contiguous int32 [B], both or neither"""
        pn, T, rows, nll_ld = _mat(nll, "nll")
        _dense(lw, torch.float64, "lw"), _dense(t0, torch.int32, "t0"), _dense(t1, torch.int32, "t1")
        for t, nm in ((logp, "logp"), (logq, "logq"), (out, "out")):
            _chk(t, torch.float64, nm)
            if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
                raise RuntimeError("iw_reduce: %s must be 2-D with contiguous rows, got shape %s strides %s" % (nm, tuple(t.shape), t.stride()))
        ldo = lambda t: t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))
        n_lat = logp.shape[0]
        if rows != B * S or tuple(logp.shape) != (n_lat, rows) or tuple(logq.shape) != (n_lat, rows) or ldo(logp) != ldo(logq) or lw.numel() != rows or (
                tuple(out.shape) != (B, _lib.FN_IW_COLS + n_lat)) or (t0 is None) != (t1 is None) or (t0 is not None and (t0.numel() != B or t1.numel() != B)):
            raise RuntimeError("iw_reduce: nll%s logp%s logq%s lw%s out%s for B %d S %d" % (
                tuple(nll.shape), tuple(logp.shape), tuple(logq.shape), tuple(lw.shape), tuple(out.shape), B, S))
        _lib.check(self.lib.fn_iw_reduce(pn, T, nll_ld, _p(t0), _p(t1), _p(logp), _p(logq), n_lat, ldo(logp), B, S, _p(lw), _p(out), ldo(out), self.stream()),
                   "fn_iw_reduce")

    @staticmethod
    def _image(t, dtype, name, N):
        """a column-major image: a 2-D view [P][>= N] with unit inner stride -> (ptr, P, n_pad)"""
        _chk(t, dtype, name)
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < N or (t.shape[1] > 1 and t.stride(1) != 1):
            raise RuntimeError("%s must be 2-D [columns][>= %d] with contiguous rows, got shape %s strides %s" % (name, N, tuple(t.shape), t.stride()))
        return _p(t), t.shape[0], (t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0)))

    def column_range(self, x, lo, hi, status):
        """fn_column_range: x a 2-D fp32 view [N][P] with unit inner stride; lo, hi contiguous fp32 [P]; status contiguous int32 [P] (the call initialises it)"""
        px, N, P, ld = _mat(x, "x")
        _dense(lo, name="lo"), _dense(hi, name="hi"), _dense(status, torch.int32, "status")
        if N < 1 or P < 1 or lo.numel() != P or hi.numel() != P or status.numel() != P:
            raise RuntimeError("column_range: x%s lo%s hi%s status%s" % (tuple(x.shape), tuple(lo.shape), tuple(hi.shape), tuple(status.shape)))
        _lib.check(self.lib.fn_column_range(px, ld, N, P, _p(lo), _p(hi), _p(status), self.stream()), "fn_column_range")

    def bin_columns(self, x, lo, hi, bins, img, status, card=None):
        """fn_bin_columns: x a 2-D fp32 view [N][P]; lo, hi contiguous fp32 [P]; img a uint8 image [P][>= N]; status contiguous int32 [P] (OR-ed into);
        card: None (all columns continuous) or P ints on the host, 0 = continuous, C = the levels 0 .. C-1"""
        px, N, P, ld = _mat(x, "x")
        _dense(lo, name="lo"), _dense(hi, name="hi"), _dense(status, torch.int32, "status")
        pi, rows, n_pad = self._image(img, torch.uint8, "img", N)
        if N < 1 or P < 1 or rows != P or lo.numel() != P or hi.numel() != P or status.numel() != P or (card is not None and len(card) != P):
            raise RuntimeError("bin_columns: x%s lo%s hi%s img%s status%s card %r" % (
                tuple(x.shape), tuple(lo.shape), tuple(hi.shape), tuple(img.shape), tuple(status.shape), card))
        arr = None if card is None else (C.c_int32 * P)(*[int(c) for c in card])
        _lib.check(self.lib.fn_bin_columns(px, ld, N, P, _p(lo), _p(hi), arr, int(bins), pi, n_pad, _p(status), self.stream()), "fn_bin_columns")

    def joint_hist(self, bz, bf, N, counts):
        """fn_joint_hist: bz, bf uint8 images [D][>= N], [A][>= N]; counts contiguous int32 [D][A][64][64] (the call zeroes it)"""
        pz, D, ldz = self._image(bz, torch.uint8, "bz", N)
        pf, A, ldf = self._image(bf, torch.uint8, "bf", N)
        _dense(counts, torch.int32, "counts")
        if N < 1 or counts.numel() != D * A * 4096:
            raise RuntimeError("joint_hist: bz%s bf%s counts%s for N %d" % (tuple(bz.shape), tuple(bf.shape), tuple(counts.shape), N))
        _lib.check(self.lib.fn_joint_hist(pz, ldz, D, pf, ldf, A, N, _p(counts), self.stream()), "fn_joint_hist")

    def column_ranks(self, x, ranks):
        """fn_column_ranks: x a 2-D fp32 view [N][P]; ranks an fp32 image [P][>= N]"""
        px, N, P, ld = _mat(x, "x")
        pr, rows, n_pad = self._image(ranks, torch.float32, "ranks", N)
        if N < 1 or P < 1 or rows != P:
            raise RuntimeError("column_ranks: x%s ranks%s" % (tuple(x.shape), tuple(ranks.shape)))
        _lib.check(self.lib.fn_column_ranks(px, ld, N, P, pr, n_pad, self.stream()), "fn_column_ranks")

    def column_corr(self, X, Y, mean_x, ss_x, mean_y, ss_y, cross):
        """fn_column_corr: X (N, P), Y (N, Q) 2-D fp32 tensors of any positive strides (a transposed image is one); mean_x, ss_x contiguous fp64 [P],
        mean_y, ss_y [Q], cross [P][Q]"""
        _chk(X, name="X"), _chk(Y, name="Y")
        if X.dim() != 2 or Y.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1 or Y.shape[1] < 1 or Y.shape[0] != X.shape[0]:
            raise RuntimeError("column_corr: X (N, P) and Y (N, Q), got %s and %s" % (tuple(X.shape), tuple(Y.shape)))
        N, P, Q = X.shape[0], X.shape[1], Y.shape[1]
        strides = [max(1, s) if n == 1 else s for t in (X, Y) for s, n in zip(t.stride(), t.shape)]          # an extent of 1 is never stepped over
        for t, n, nm in ((mean_x, P, "mean_x"), (ss_x, P, "ss_x"), (mean_y, Q, "mean_y"), (ss_y, Q, "ss_y"), (cross, P * Q, "cross")):
            _dense(t, torch.float64, nm)
            if t.numel() != n:
                raise RuntimeError("column_corr: %s holds %d entries, not %d" % (nm, t.numel(), n))
        if min(strides) < 1:
            raise RuntimeError("column_corr: positive strides, got %s and %s" % (X.stride(), Y.stride()))
        _lib.check(self.lib.fn_column_corr(_p(X), strides[0], strides[1], P, _p(Y), strides[2], strides[3], Q, N, _p(mean_x), _p(ss_x), _p(mean_y),
                                           _p(ss_y), _p(cross), self.stream()), "fn_column_corr")

    def mi_scores(self, counts, out, hits):
        """fn_mi_scores: counts contiguous int32 [pairs][64][64]; out contiguous fp64 [pairs][3] (I, H_z, H_f); hits contiguous int32 [pairs]"""
        _dense(counts, torch.int32, "counts"), _dense(out, torch.float64, "out"), _dense(hits, torch.int32, "hits")
        pairs = hits.numel()
        if pairs < 1 or counts.numel() != pairs * 4096 or out.numel() != pairs * _lib.FN_DIS_MI_COLS:
            raise RuntimeError("mi_scores: counts%s out%s hits%s" % (tuple(counts.shape), tuple(out.shape), tuple(hits.shape)))
        _lib.check(self.lib.fn_mi_scores(_p(counts), pairs, _p(out), _p(hits), self.stream()), "fn_mi_scores")

    def sweep_scores(self, r, n, status, values, which, r_std, n_std, scores, n_used):
        """fn_sweep_scores: r, n fp32 and status int32 contiguous [S][Vn]; values fp64 [Vn]; scores fp64 [4]; n_used int32 [1]"""
        _dense(r, name="r"), _dense(n, name="n"), _dense(status, torch.int32, "status"), _dense(values, torch.float64, "values")
        _dense(scores, torch.float64, "scores"), _dense(n_used, torch.int32, "n_used")
        if r.dim() != 2 or n.shape != r.shape or status.shape != r.shape or values.numel() != r.shape[1] or scores.numel() != 4 or n_used.numel() != 1:
            raise RuntimeError("sweep_scores: r, n, status [S][Vn], values [Vn], scores [4], n_used [1]; got %s %s %s %d" % (
                tuple(r.shape), tuple(n.shape), tuple(status.shape), values.numel()))
        _lib.check(self.lib.fn_sweep_scores(_p(r), _p(n), _p(status), r.shape[0], r.shape[1], _p(values), int(which), float(r_std), float(n_std), _p(scores),
                                            _p(n_used), self.stream()), "fn_sweep_scores")

    def token_score(self, x, stride_b, stride_t, B, T, V, target=None, pred=None, nll=None, rank=None):
        """fn_token_score: row (b, t) = the V floats at x.data_ptr() + 4 (b stride_b + t stride_t), which must lie inside x's storage; target int32
        (B, >= T) and the outputs pred, rank int32 / nll fp32 (B, >= T), each optional, with contiguous rows; the outputs share one row stride"""
        _chk(x, name="x"), _chk(target, torch.int32, "target"), _chk(pred, torch.int32, "pred"), _chk(nll, name="nll"), _chk(rank, torch.int32, "rank")
        B, T, V, stride_b, stride_t = int(B), int(T), int(V), int(stride_b), int(stride_t)
        room = x.untyped_storage().nbytes() // 4 - x.storage_offset()
        if min(B, T, V) < 1 or min(stride_b, stride_t) < 0 or (B - 1) * stride_b + (T - 1) * stride_t + V > room:
            raise RuntimeError("token_score: rows of %d floats at strides (%d, %d) for B = %d, T = %d do not fit the %d floats behind x" % (V, stride_b, stride_t, B, T, room))
        lds = set()
        for t, nm in ((target, "target"), (pred, "pred"), (nll, "nll"), (rank, "rank")):
            if t is None:
                continue
            if t.dim() != 2 or t.shape[0] != B or t.shape[1] < T or (t.shape[1] > 1 and t.stride(1) != 1) or (B > 1 and t.stride(0) < T):
                raise RuntimeError("token_score: %s (%d, >= %d) with contiguous rows, got shape %s strides %s" % (nm, B, T, tuple(t.shape), t.stride()))
            if nm != "target":
                lds.add(t.stride(0) if B > 1 else max(t.shape[1], t.stride(0)))
        if len(lds) != 1:
            raise RuntimeError("token_score: at least one of pred, nll, rank, and one row stride for all of them (got %s)" % sorted(lds))
        tgt_ld = 0 if target is None else (target.stride(0) if B > 1 else max(target.shape[1], target.stride(0)))
        _lib.check(self.lib.fn_token_score(_p(x), stride_b, stride_t, B, T, V, _p(target), tgt_ld, _p(pred), _p(nll), _p(rank), lds.pop(), self.stream()),
                   "fn_token_score")

    def match_rows(self, pred, target, T, trim, lead, len_, correct, acc, status, nll=None, rank=None, topk=1, correct_topk=None, nll_sum=None):
        """fn_match_rows: pred, target int32 (rows, >= T) with contiguous rows; nll fp32 / rank int32 (rows, >= T) sharing one row stride, or None;
        lead, len_, correct, status, correct_topk int32 [rows], acc, nll_sum fp64 [rows]"""
        rows, T = pred.shape[0], int(T)
        ld = {}
        for t, d, nm in ((pred, torch.int32, "pred"), (target, torch.int32, "target"), (nll, torch.float32, "nll"), (rank, torch.int32, "rank")):
            _chk(t, d, nm)
            if t is None:
                continue
            if t.dim() != 2 or t.shape[0] != rows or t.shape[1] < T or T < 1 or (t.shape[1] > 1 and t.stride(1) != 1) or (rows > 1 and t.stride(0) < T):
                raise RuntimeError("match_rows: %s (%d, >= %d) with contiguous rows, got shape %s strides %s" % (nm, rows, T, tuple(t.shape), t.stride()))
            ld[nm] = t.stride(0) if rows > 1 else max(t.shape[1], t.stride(0))
        if nll is not None and rank is not None and ld["nll"] != ld["rank"]:
            raise RuntimeError("match_rows: nll and rank share one row stride, got %d and %d" % (ld["nll"], ld["rank"]))
        for t, d, nm in ((lead, torch.int32, "lead"), (len_, torch.int32, "len"), (correct, torch.int32, "correct"), (status, torch.int32, "status"),
                         (correct_topk, torch.int32, "correct_topk"), (acc, torch.float64, "acc"), (nll_sum, torch.float64, "nll_sum")):
            _dense(t, d, nm)
            if t is not None and t.numel() != rows:
                raise RuntimeError("match_rows: %s for %d rows" % (nm, rows))
        _lib.check(self.lib.fn_match_rows(_p(pred), ld["pred"], _p(target), ld["target"], rows, T, 1 if trim else 0, _p(nll), _p(rank),
                                          ld.get("nll", ld.get("rank", 0)), int(topk), _p(lead), _p(len_), _p(correct), _p(correct_topk), _p(acc),
                                          _p(nll_sum), _p(status), self.stream()), "fn_match_rows")

    def time_logsoftmax(self, logits, logp_bt=None, target=None, nll_bc=None, grad_scale=0.0, dlogits=None):
        _dense(logits, name="logits"), _dense(logp_bt, name="logp_bt"), _dense(target, torch.int32, "target")
        _dense(nll_bc, name="nll_bc"), _dense(dlogits, name="dlogits")
        Tr, B, Cc = logits.shape
        _lib.check(self.lib.fn_time_logsoftmax(_p(logits), B, Tr, Cc, _p(logp_bt), _p(target), _p(nll_bc), grad_scale, _p(dlogits),
                                               self.stream()), "fn_time_logsoftmax")

    def time_logsoftmax_bwd(self, logp_bt, gout_bt, dlogits):
        _dense(logp_bt, name="logp_bt"), _dense(gout_bt, name="gout_bt"), _dense(dlogits, name="dlogits")
        B, Tr, Cc = logp_bt.shape
        _lib.check(self.lib.fn_time_logsoftmax_bwd(_p(logp_bt), _p(gout_bt), B, Tr, Cc, _p(dlogits), self.stream()), "fn_time_logsoftmax_bwd")

    # -- latent ---------------------------------------------------------------------------------
    def latent_fwd(self, pre, eps, mu_lk, lv_lk, labels, sigma, z, ll, qy, y, terms):
        for t, n in ((pre, "pre"), (eps, "eps"), (mu_lk, "mu_lk"), (lv_lk, "lv_lk"), (sigma, "sigma"), (z, "z"), (ll, "ll"), (qy, "qy"),
                     (terms, "terms")):
            _dense(t, name=n)
        _dense(labels, torch.int32, "labels"), _dense(y, torch.int32, "y")
        B, Z = eps.shape
        K = mu_lk.shape[0]
        _lib.check(self.lib.fn_latent_fwd(_p(pre), _p(eps), _p(mu_lk), _p(lv_lk), B, Z, K, _p(labels), _p(sigma), _p(z), _p(ll), _p(qy),
                                          _p(y), _p(terms), self.stream()), "fn_latent_fwd")

    def latent_bwd(self, pre, eps, mu_lk, lv_lk, labels, z, qy, g_z, g_mu, g_sigma, g_ll, g_qy, w3, dpre, dmu_lk_rows):
        """w3: device float tensor {w_lat, w_cls, w_clf} (see fn_step_params) or None (= zeros)"""
        for t, n in ((pre, "pre"), (eps, "eps"), (mu_lk, "mu_lk"), (lv_lk, "lv_lk"), (z, "z"), (qy, "qy"), (g_z, "g_z"), (g_mu, "g_mu"),
                     (g_sigma, "g_sigma"), (g_ll, "g_ll"), (g_qy, "g_qy"), (dpre, "dpre"), (dmu_lk_rows, "dmu_lk_rows"), (w3, "w3")):
            _dense(t, name=n)
        _dense(labels, torch.int32, "labels")
        B, Z = eps.shape
        K = mu_lk.shape[0]
        _lib.check(self.lib.fn_latent_bwd(_p(pre), _p(eps), _p(mu_lk), _p(lv_lk), B, Z, K, _p(labels), _p(z), _p(qy), _p(g_z), _p(g_mu),
                                          _p(g_sigma), _p(g_ll), _p(g_qy), _p(w3), _p(dpre), _p(dmu_lk_rows),
                                          self.stream()), "fn_latent_bwd")

    def masked_prob(self, logits, E, ranges, sums=None, w=None, dlogits=None):
        """softmax mass of two token ranges per logits row (fn_masked_prob) and / or the gradient of w0 P_0 + w1 P_1 wrt the logits"""
        pl, rows, _, ld = _mat(logits, "logits")
        _dense(sums, name="sums"), _dense(w, name="w")
        pd = None
        if dlogits is not None:
            pd, r2, _, ld2 = _mat(dlogits, "dlogits")
            if (r2, ld2) != (rows, ld):
                raise RuntimeError("masked_prob: dlogits must have the layout of logits")
        (lo0, hi0), (lo1, hi1) = ranges
        _lib.check(self.lib.fn_masked_prob(pl, rows, E, ld, lo0, hi0, lo1, hi1, _p(sums), _p(w), pd, self.stream()), "fn_masked_prob")

    def adv_head(self, z, w_r, w_n, b_r, b_n, mask, dens, lam_dev, inv_global_batch, o, loss_rows, da=None, g_z=None):
        """adversarial heads of the Fader sibling (fn_adv_head): z [B][>=Z] row view, g_z likewise (gradient is SUBTRACTED)"""
        pz, B, Zc, ldz = _mat(z, "z")
        for t, nm in ((w_r, "w_r"), (w_n, "w_n"), (b_r, "b_r"), (b_n, "b_n"), (mask, "mask"), (dens, "dens"), (o, "o"), (loss_rows, "loss_rows"),
                      (da, "da"), (lam_dev, "lam_dev")):
            _dense(t, name=nm)
        Z = w_r.numel()
        if Zc < Z or tuple(mask.shape) != (B, 2) or tuple(dens.shape) != (B, 2):
            raise RuntimeError("adv_head shape mismatch")
        pg, ldg = (None, 0)
        if g_z is not None:
            pg, _, _, ldg = _mat(g_z, "g_z")
        _lib.check(self.lib.fn_adv_head(pz, ldz, Z, B, _p(w_r), _p(w_n), _p(b_r), _p(b_n), _p(mask), _p(dens), _p(lam_dev), inv_global_batch,
                                        _p(o), _p(loss_rows), _p(da), pg, ldg, self.stream()), "fn_adv_head")

    def pairwise_reg(self, z0_all, attr_all, row0, nrows, loss_rows, grad_scale=0.0, dz0=None):
        _dense(z0_all, name="z0_all"), _dense(attr_all, torch.float64, "attr_all"), _dense(loss_rows, name="loss_rows"), _dense(dz0, name="dz0")
        _lib.check(self.lib.fn_pairwise_reg(_p(z0_all), _p(attr_all), z0_all.numel(), row0, nrows, _p(loss_rows), grad_scale, _p(dz0),
                                            self.stream()), "fn_pairwise_reg")

    # -- optimiser ------------------------------------------------------------------------------
    def sumsq(self, g, out):
        _dense(g, name="g"), _chk(out, name="out")
        wsb = self.lib.fn_sumsq_ws_bytes(g.numel())
        ws = self.workspace(wsb, "sumsq")
        _lib.check(self.lib.fn_sumsq_f32(_p(g), g.numel(), _p(out), _p(ws), wsb, self.stream()), "fn_sumsq_f32")

    def step_params(self, counters, beta, lr, beta1, beta2, supervised, inv_global_batch, advance, out):
        """device-resident step counters -> {w_lat, w_cls, w_clf, lr/(1-b1^t), 1/sqrt(1-b2^t), beta0} (see fn_step_params)"""
        _dense(counters, torch.int64, "counters"), _dense(out, name="out")
        if counters.numel() < 2 or out.numel() < 8:
            raise RuntimeError("step_params: counters[2] / out[8] expected")
        _lib.check(self.lib.fn_step_params(_p(counters), beta, lr, beta1, beta2, int(supervised), inv_global_batch, int(advance), _p(out),
                                           self.stream()), "fn_step_params")

    def clip_adam(self, p, g, m, v, sumsq, max_norm, hyper, beta1, beta2, eps):
        for t, n in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
            _dense(t, name=n)
        _chk(sumsq, name="sumsq"), _chk(hyper, name="hyper")
        _lib.check(self.lib.fn_clip_adam(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(sumsq), max_norm, _p(hyper), beta1, beta2, eps,
                                         self.stream()), "fn_clip_adam")

    def onehot_to_index(self, oh, idx):
        _dense(oh, name="oh"), _dense(idx, torch.int32, "idx")
        V = oh.shape[-1]
        _lib.check(self.lib.fn_onehot_to_index(_p(oh), oh.numel() // V, V, _p(idx), self.stream()), "fn_onehot_to_index")
