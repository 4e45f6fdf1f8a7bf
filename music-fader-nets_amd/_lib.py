"""ctypes binding of libfadernets_hip.so (the C ABI in include/fadernets.h).

The product path has NO fallback: if the library is missing or a symbol is absent this module
raises, and every op in hipops.py raises on a non-zero return code.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfadernets_hip.so")

FN_MAX_SCANS = 8
ABI_VERSION = 6
GEMM_LEAN = 0x10000          # FN_GEMM_LEAN
GEMM_BF16X6 = 0x20000        # FN_GEMM_BF16X6 (exact bf16 triple split on the bf16 MFMA)
GEMM_X6_WIDE = 0x80000       # FN_GEMM_X6_WIDE (128 x 256 output tiles per workgroup)
GEMM_X6_PERTILE = 0x100000   # FN_GEMM_X6_PERTILE (tests / A-B: one workgroup per tile / (tile, K range) item instead of one per CU walking its items)
GEMM_X6_PERWAVE = 0x40000    # FN_GEMM_X6_PERWAVE (tests / A-B: the round-5 kernel, every wavefront splits its own operands)
# FnGruFwd / FnGruBwd / FnGruCell .variant bits (FN_GRU_* in include/fadernets.h)
# FnGemmPlan.kernel -> the kernel instance (enum FnGemmKernel of include/fadernets.h, in its order) and FnGemmPlan.reduce -> the slab reduction
GEMM_PLAN_KERNELS = ("gemm_kernel<64,64,16>", "gemm_kernel<64,64,32>", "gemm_kernel<32,64,32>", "gemm_kernel<64,16,16>", "gemm_kernel<128,128,32>",
                     "gemm_nt_direct_kernel<4, 2>", "gemm_nt_direct_kernel<1, 4>", "gemm_nt_x6w_kernel", "gemm_tn_kernel", "gemm_tn_lean_kernel",
                     "gemm_tn_x6_kernel", "gemm_tn_x6w_kernel", "gemm_tn_x6v_kernel")
GEMM_PLAN_REDUCES = (None, "slab_reduce_kernel", "slab_reduce4_kernel")
# FnGruCandidate.kernel -> the kernel instance (enum FnGruKernel, in its order), FnGruPlan.ws_absent (enum FnGruAbsent), FnGruCellPlan.family
GRU_PLAN_KERNELS = ("gru_fwd_x6pp_kernel<1>", "gru_fwd_x6pp_kernel<2>", "gru_fwd_x6_kernel<1>", "gru_fwd_x6_kernel<2>", "gru_fwd_pp_kernel<1>",
                    "gru_fwd_pp_kernel<2>", "gru_fwd_persist_kernel<4, 1, 2, 4>", "gru_fwd_persist_kernel<4, 1, 1, 4>", "gru_fwd_persist_kernel<2, 2, 2, 4>",
                    "gru_fwd_persist_kernel<2, 2, 1, 4>", "gru_fwd_persist_kernel<1, 4, 1, 4>", "gru_fwd_step_kernel",
                    "gru_bwd_x6_kernel<1>", "gru_bwd_x6_kernel<2>", "gru_bwd_rs_kernel<1>", "gru_bwd_rs_kernel<2>", "gru_bwd_persist_kernel<4, 1, 2, 8>",
                    "gru_bwd_persist_kernel<4, 1, 1, 8>", "gru_bwd_persist_kernel<2, 2, 2, 8>", "gru_bwd_persist_kernel<2, 2, 1, 8>",
                    "gru_bwd_persist_kernel<1, 4, 1, 8>", "gru_bwd_step_kernel")
GRU_PLAN_ABSENT = (None, "H > 512", "no sync_ws", "mixed H", "unaligned", "T < 2", "slices > cus", "no row block")
GRU_CELL_FAMILIES = ("staged", "direct", "wlds", "wlds-overlap", "x6")
# FnOutArgmaxPlan.kernel -> the kernel instance (enum FnOutArgmaxKernel, in its order)
OUT_ARGMAX_KERNELS = ("out_argmax_lds8_kernel<4>", "out_argmax_lds_kernel<8>", "out_argmax_direct_kernel<4>")
GRU_ROWS_MASK = 0xFF         # forced rows per workgroup (scans) / forced form 1-18 (cells)
GRU_ALT_TILING = 0x100       # the alternative wave tiling of the 64-row configuration
GRU_SYNC_ZEROED = 0x200      # the sync_ws counters are already zero
GRU_COMPILER_LOOPS = 0x400   # compiler-scheduled K loops
GRU_NO_PINGPONG = 0x800      # the round-3 loops
GRU_SPREAD_XCDS = 0x1000     # every row group spread over all XCDs (placement test)
GRU_NO_RS_BWD = 0x2000       # backward: not the register-stationary kernel
GRU_BF16X6 = 0x4000          # bf16 x 6 scans / cell
GRU_X6_SINGLE_GROUP = 0x8000  # with GRU_BF16X6, forward: the single-group kernel (no ping-pong)
GRU_X6_BWD_32ROWS = 0x8000   # with GRU_BF16X6, backward: 32-row groups eligible too
FN_E_NULL, FN_E_SHAPE, FN_E_ALIGN, FN_E_WORKSPACE, FN_E_COUNT = -1, -2, -3, -4, -5
FN_E_UNSUPPORTED = -6
FN_E_COMM = -7
FN_COMM_ID_BYTES = 128
FN_COLSUM_MAX_JOBS = 64
FN_SAMPLE_MAX_V = 1024
FN_BEAM_MAX_W = 16
FN_BEAM_GATHER_MAX_JOBS = 4
CONSTRAIN_OFF_NEEDS_ON = 1      # FN_CONSTRAIN_OFF_NEEDS_ON
CONSTRAIN_NO_REONSET = 2        # FN_CONSTRAIN_NO_REONSET
FN_CONSTRAIN_MAX_PITCH = 128
FN_ATTR_MAX_STEPS, FN_ATTR_MAX_CELLS, FN_ATTR_MAX_SAMPLES = 1024, 2048, 4096
FN_ATTR_EMPTY, FN_ATTR_OVERFLOW = 1, 2
FN_NOTES_MAX, FN_NOTES_MAX_TICK = 512, 1 << 22
FN_NOTES_EMPTY, FN_NOTES_OVERFLOW = 1, 2
FN_STITCH_MAX_S, FN_STITCH_MAX_V, FN_STITCH_MAX_OUT = 1 << 16, 64, 1 << 24
FN_DRAW_MAX_JOBS, FN_DRAW_MAX_Z, FN_DRAW_MAX_K = 4, 4096, 1024
FN_MIX_LERP, FN_MIX_SLERP, FN_MIX_STEP = 0, 1, 2
FN_MIX_MAX_SEGS, FN_MIX_MIN_SIN = 4, 1e-4
FN_MATCH_EMPTY = 1
FN_POST_MAX_K, FN_IW_MAX_LAT, FN_IW_COLS = 8, 4, 4
FN_DIS_MAX_N, FN_DIS_MAX_D, FN_DIS_MAX_A, FN_DIS_MAX_BINS = 1 << 22, 4096, 16, 64
FN_DIS_RANGE_CHUNK, FN_DIS_HIST_CHUNK, FN_DIS_RANK_ROWS, FN_DIS_RANK_TILE = 1024, 4096, 1024, 1024
FN_DIS_NONFINITE, FN_DIS_BAD_LEVEL, FN_DIS_MI_COLS = 1, 2, 3
_f =C.POINTER(C.c_float)
_i = C.POINTER(C.c_int32)
vp = C.c_void_p


class FnGruFwd(C.Structure):
    _fields_ = [("B", C.c_int32), ("T", C.c_int32), ("H", C.c_int32), ("reverse", C.c_int32),
                ("w_hh_frag", vp), ("b_hh", vp), ("b_ih", vp), ("h0", vp), ("gx_dense", vp), ("gx_table", vp),
                ("idx", vp), ("idx_ld", C.c_int32), ("idx_shift", C.c_int32), ("start_token", C.c_int32),
                ("gx_rowbias", vp), ("h_all", vp), ("gates", vp), ("frag_ws", vp), ("sync_ws", vp), ("cu_budget", C.c_int32), ("h0_frag", vp), ("h_last_frag", vp), ("variant", C.c_int32), ("err_ws", vp)]


class FnGruBwd(C.Structure):
    _fields_ = [("B", C.c_int32), ("T", C.c_int32), ("H", C.c_int32),
                ("w_hh_t_frag", vp), ("h0", vp), ("h_all", vp), ("gates", vp), ("dh_last", vp), ("dh_ext", vp),
                ("dgx_all", vp), ("dghn_all", vp), ("dh0", vp), ("dgx_rowsum", vp), ("dghn_rowsum", vp), ("scratch", vp), ("frag_ws", vp),
                ("sync_ws", vp), ("cu_budget", C.c_int32), ("variant", C.c_int32), ("err_ws", vp)]


class FnEmbedGrad(C.Structure):
    _fields_ = [("dgx_all", vp), ("out", vp), ("out_ld", C.c_int32), ("transposed", C.c_int32), ("reverse", C.c_int32),
                ("idx_shift", C.c_int32), ("start_token", C.c_int32)]


class FnGemmSeg(C.Structure):
    _fields_ = [("A", vp), ("lda", C.c_int32), ("B", vp), ("ldb", C.c_int32), ("K", C.c_int32)]


class FnGemmJob(C.Structure):
    _fields_ = [("M", C.c_int32), ("N", C.c_int32), ("seg", FnGemmSeg * 4), ("n_seg", C.c_int32), ("beta", C.c_float), ("C", vp),
                ("ldc", C.c_int32), ("bias", vp)]


class FnGemmPlan(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("klen", C.c_int32), ("ranges", C.c_int32), ("grid_x", C.c_int32), ("grid_y", C.c_int32), ("grid_z", C.c_int32),
                ("tiles", C.c_int32), ("reduce", C.c_int32), ("reduce_blocks", C.c_int32), ("msplit", C.c_int32)]

    def as_dict(self):
        """kernel and reduce by name, grid as (x, y, z)"""
        return dict(kernel=GEMM_PLAN_KERNELS[self.kernel], klen=self.klen, ranges=self.ranges, grid=(self.grid_x, self.grid_y, self.grid_z), tiles=self.tiles,
                    reduce=GEMM_PLAN_REDUCES[self.reduce], reduce_blocks=self.reduce_blocks, msplit=self.msplit)


class FnGruCandidate(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("kernel", "rows_per_group", "groups", "slices", "grid", "lds_bytes", "no_hand", "h0_triples", "resident", "fits",
                                         "tm", "tn", "d", "ns", "tiles", "launches")]

    def as_dict(self):
        """kernel by name; fits: True / False / None (not asked)"""
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d.update(kernel=GRU_PLAN_KERNELS[self.kernel], fits=None if self.fits < 0 else bool(self.fits))
        return d


class FnGruPlan(C.Structure):
    _fields_ = [("status", C.c_int32), ("n", C.c_int32), ("chosen", C.c_int32), ("cus", C.c_int32), ("ws_absent", C.c_int32), ("cand", FnGruCandidate * 3)]

    def as_dict(self):
        """candidates in the order the launch tries them; chosen: index of the one it takes (None: not known / none)"""
        return dict(status=self.status, chosen=None if self.chosen < 0 else self.chosen, cus=self.cus, ws_absent=GRU_PLAN_ABSENT[self.ws_absent],
                    candidates=[self.cand[i].as_dict() for i in range(self.n)])


class FnGruCellPlan(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("status", "family", "t0", "t1", "t2", "has_tab", "has_rb", "kmax", "grid", "threads", "lds_bytes", "forced_honoured")]

    def as_dict(self):
        """family by name, template arguments as a tuple"""
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d.update(family=GRU_CELL_FAMILIES[self.family], template=(self.t0, self.t1, self.t2), forced_honoured=bool(self.forced_honoured))
        return d


class FnColsumJob(C.Structure):
    _fields_ = [("X", vp), ("M", C.c_int32), ("N", C.c_int32), ("ld", C.c_int32), ("beta", C.c_float), ("out", vp)]


class FnGruCell(C.Structure):
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("x", vp), ("ldx", C.c_int32), ("K1", C.c_int32), ("w_ih", vp), ("ldw_ih", C.c_int32),
                ("gx_table", vp), ("idx", vp), ("idx_ld", C.c_int32), ("start_token", C.c_int32), ("gx_rowbias", vp), ("h_prev", vp),
                ("ldh", C.c_int32), ("w_hh", vp), ("ldw_hh", C.c_int32), ("b_ih", vp), ("b_hh", vp), ("h_out", vp), ("ldo", C.c_int32), ("variant", C.c_int32),
                ("idx_best", vp), ("best_v", C.c_int32)]


class FnWeightImage(C.Structure):
    _fields_ = [("src", vp), ("dst", vp), ("rows", C.c_int32), ("cols", C.c_int32), ("ld", C.c_int32), ("kind", C.c_int32)]


class FnDecode(C.Structure):
    _fields_ = [("B", C.c_int32), ("steps", C.c_int32), ("H", C.c_int32), ("V", C.c_int32), ("start_token", C.c_int32),
                ("w_hh1_frag", vp), ("b_hh1", vp), ("b_ih1", vp), ("table1", vp), ("rowbias1", vp), ("h0", vp),
                ("w_ih2_frag", vp), ("b_ih2", vp), ("w_hh2_frag", vp), ("b_hh2", vp), ("w_out_frag", vp), ("b_out", vp),
                ("tokens", vp), ("tok_ld", C.c_int32), ("logp", vp), ("ws", vp), ("sync_ws", vp)]


class FnDecodeForce(C.Structure):
    _fields_ = [("forced", vp), ("forced_ld", C.c_int32), ("force", vp)]


class FnDecodePlan(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("status", "forced", "mt", "block_rows", "nblk", "nvt", "nslices", "per_rep", "nrep", "grid", "threads", "lds_bytes")] + [
        (k, C.c_int64) for k in ("x1_off", "x2_off", "g2_off", "logits_off", "ws_floats")]

    def as_dict(self):
        """every field by name; forced as a bool"""
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d.update(forced=bool(self.forced))
        return d


class FnOutArgmaxPlan(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("status", "kernel", "grid", "threads", "lds_bytes")]

    def as_dict(self):
        """kernel by name"""
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d.update(kernel=OUT_ARGMAX_KERNELS[self.kernel])
        return d


class FnSampleParams(C.Structure):
    _fields_ = [("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("offset_lo", C.c_uint32), ("offset_hi", C.c_uint32),
                ("inv_temperature", C.c_float), ("top_p", C.c_float), ("top_k", C.c_int32), ("reserved", C.c_int32)]


class FnBeamGatherJob(C.Structure):
    _fields_ = [("src", vp), ("src_ld", C.c_int32), ("dst", vp), ("dst_ld", C.c_int32), ("cols", C.c_int32)]


class FnConstrainParams(C.Structure):
    _fields_ = [("on_lo", C.c_int32), ("off_lo", C.c_int32), ("n_pitch", C.c_int32), ("max_poly", C.c_int32), ("eos", C.c_int32),
                ("min_len", C.c_int32), ("flags", C.c_uint32), ("reserved", C.c_int32)]


class FnAttrParams(C.Structure):
    _fields_ = [("on_lo", C.c_int32), ("off_lo", C.c_int32), ("n_pitch", C.c_int32), ("shift_lo", C.c_int32), ("n_shift", C.c_int32), ("eos", C.c_int32),
                ("ticks_num", C.c_int32), ("ticks_den", C.c_int32), ("beat_cells", C.c_int32), ("vocab_size", C.c_int32), ("reserved", C.c_int32 * 2)]


class FnNote(C.Structure):
    _fields_ = [("t0", C.c_int32), ("t1", C.c_int32), ("pitch", C.c_int32), ("vel", C.c_int32)]


class FnNoteSpan(C.Structure):
    _fields_ = [("first", C.c_int32), ("count", C.c_int32), ("t_lo", C.c_int32), ("t_hi", C.c_int32)]


class FnNoteParams(C.Structure):
    _fields_ = [("on_lo", C.c_int32), ("off_lo", C.c_int32), ("n_pitch", C.c_int32), ("shift_lo", C.c_int32), ("n_shift", C.c_int32), ("eos", C.c_int32),
                ("vocab_size", C.c_int32), ("vel_lo", C.c_int32), ("n_vel", C.c_int32), ("default_vel", C.c_int32), ("pad", C.c_int32),
                ("add_eos", C.c_int32), ("reserved", C.c_int32 * 4)]


class FnDrawParams(C.Structure):
    _fields_ = [("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("offset_lo", C.c_uint32), ("offset_hi", C.c_uint32), ("tau", C.c_float),
                ("reserved", C.c_int32 * 3)]


class FnDrawJob(C.Structure):
    _fields_ = [("mu_lk", vp), ("lv_lk", vp), ("comp", vp), ("z", vp), ("eps_out", vp), ("comp_out", vp), ("K", C.c_int32), ("stream_id", C.c_int32)]


class FnPostJob(C.Structure):
    _fields_ = [("pre", vp), ("mu_lk", vp), ("lv_lk", vp), ("z", vp), ("eps_out", vp), ("logq", vp), ("logp", vp), ("K", C.c_int32), ("stream_id", C.c_int32)]


class FnMixSeg(C.Structure):
    _fields_ = [("off", C.c_int32), ("len", C.c_int32), ("mode", C.c_int32), ("reserved", C.c_int32)]


# name -> (restype, argtypes); every symbol declared in include/fadernets.h
SIGNATURES = {
    "fn_version": (C.c_int, []),
    "fn_strerror": (C.c_char_p, [C.c_int]),
    "fn_frag3_pack": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "fn_gemm_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "fn_gemm_f32": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, vp, C.c_int, vp, C.c_int,
                              C.c_float, vp, C.c_int, vp, C.c_int, vp, C.c_size_t, vp]),
    "fn_gemm_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int,
                               C.POINTER(FnGemmPlan)]),
    "fn_gemm_multi": (C.c_int, [C.c_int, C.c_int, C.POINTER(FnGemmJob), C.c_int, vp]),
    "fn_transpose_f32": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
    "fn_colsum_ws_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "fn_colsum_f32": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_float, vp, vp, C.c_size_t, vp]),
    "fn_colsum_multi": (C.c_int, [C.POINTER(FnColsumJob), C.c_int, vp]),
    "fn_axpy_f32": (C.c_int, [C.c_int64, C.c_float, vp, vp, vp]),
    "fn_sum_f32": (C.c_int, [vp, C.c_int64, C.c_float, vp, vp]),
    "fn_gru_gates_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "fn_frag_floats": (C.c_size_t, [C.c_int, C.c_int]),
    "fn_frag_pack": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "fn_weight_images": (C.c_int, [C.POINTER(FnWeightImage), C.c_int, vp]),
    "fn_gru_sync_ws_bytes": (C.c_size_t, []),
    "fn_gru_seq_fwd": (C.c_int, [C.POINTER(FnGruFwd), C.c_int, vp]),
    "fn_gru_fwd_x6_ok": (C.c_int, [C.POINTER(FnGruFwd), C.c_int]),
    "fn_gru_cell_f32": (C.c_int, [C.POINTER(FnGruCell), vp]),
    "fn_gru_fwd_plan": (C.c_int, [C.POINTER(FnGruFwd), C.c_int, C.c_int, C.POINTER(FnGruPlan)]),
    "fn_gru_bwd_plan": (C.c_int, [C.POINTER(FnGruBwd), C.c_int, C.c_int, C.POINTER(FnGruPlan)]),
    "fn_gru_cell_plan": (C.c_int, [C.POINTER(FnGruCell), C.POINTER(FnGruCellPlan)]),
    "fn_out_argmax_f32": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "fn_out_argmax_plan": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, C.POINTER(FnOutArgmaxPlan)]),
    "fn_best_tokens": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp]),
    "fn_gru_seq_bwd": (C.c_int, [C.POINTER(FnGruBwd), C.c_int, vp]),
    "fn_gru_bwd_x6_ok": (C.c_int, [C.POINTER(FnGruBwd), C.c_int]),
    "fn_decode_ws_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "fn_decode_sync_ws_bytes": (C.c_size_t, []),
    "fn_decode_greedy": (C.c_int, [C.POINTER(FnDecode), vp]),
    "fn_decode_forced": (C.c_int, [C.POINTER(FnDecode), C.POINTER(FnDecodeForce), vp]),
    "fn_decode_plan": (C.c_int, [C.POINTER(FnDecode), C.POINTER(FnDecodeForce), C.c_int, C.POINTER(FnDecodePlan)]),
    "fn_gru_dwhh_ws_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "fn_gru_dwhh_f32": (C.c_int, [vp, vp, vp, C.c_int64, C.c_int, C.c_float, vp, C.c_int, vp, C.c_size_t, vp]),
    "fn_gru_dwhh_plan": (C.c_int, [vp, vp, vp, vp, vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(FnGemmPlan)]),
    "fn_embed_grad_ws_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "fn_embed_grad_f32": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                    vp, vp, C.c_size_t, vp]),
    "fn_token_sort_ints": (C.c_size_t, [C.c_int64, C.c_int]),
    "fn_token_sort_ws_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "fn_token_sort": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_size_t, vp]),
    "fn_embed_grad_sorted_ws_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]),
    "fn_embed_grad_sorted": (C.c_int, [C.POINTER(FnEmbedGrad), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_size_t, vp]),
    "fn_time_sum_f32": (C.c_int, [vp, C.c_int, C.c_int64, vp, vp]),
    "fn_vocab_logsoftmax": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_float, vp, vp]),
    "fn_vocab_logsoftmax_bwd": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]),
    "fn_out_head_f32": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_float, vp, vp, C.c_int, vp]),
    "fn_vocab_argmax": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int64, vp, C.c_int, vp]),
    "fn_vocab_sample": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, C.c_int64, vp, C.c_int, vp, C.c_int, vp, vp]),
    "fn_beam_step": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int64, vp]),
    "fn_beam_gather": (C.c_int, [C.POINTER(FnBeamGatherJob), C.c_int, C.c_int, C.c_int, vp, vp]),
    "fn_beam_backtrack": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]),
    "fn_constrain_apply": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int64, vp, vp, vp]),
    "fn_constrain_advance": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, vp, vp, vp]),
    "fn_event_attributes": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]),
    "fn_sweep_scores": (C.c_int, [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_double, C.c_double, vp, vp, vp]),
    "fn_notes_from_tokens": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp]),
    "fn_tokens_from_notes": (C.c_int, [vp, C.c_int, vp, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]),
    "fn_notes_stitch": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp, vp]),
    "fn_latent_draw": (C.c_int, [C.POINTER(FnDrawJob), C.c_int, C.c_int, C.c_int, C.c_int64, vp, vp]),
    "fn_latent_mix": (C.c_int, [vp, vp, C.c_int64, C.c_int, C.c_int, vp, C.c_int, C.c_int, C.POINTER(FnMixSeg), C.c_int, vp, C.c_int64, vp, vp]),
    "fn_posterior_draw": (C.c_int, [C.POINTER(FnPostJob), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, vp, vp]),
    "fn_iw_reduce": (C.c_int, [vp, C.c_int, C.c_int64, vp, vp, vp, vp, C.c_int, C.c_int64, C.c_int, C.c_int, vp, vp, C.c_int, vp]),
    "fn_column_range": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, vp, vp, vp, vp]),
    "fn_bin_columns": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, vp, vp, _i, C.c_int, vp, C.c_int64, vp, vp]),
    "fn_joint_hist": (C.c_int, [vp, C.c_int64, C.c_int, vp, C.c_int64, C.c_int, C.c_int, vp, vp]),
    "fn_column_ranks": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, vp, C.c_int64, vp]),
    "fn_column_corr": (C.c_int, [vp, C.c_int64, C.c_int64, C.c_int, vp, C.c_int64, C.c_int64, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]),
    "fn_mi_scores": (C.c_int, [vp, C.c_int, vp, vp, vp]),
    "fn_token_score": (C.c_int, [vp, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, C.c_int, vp]),
    "fn_match_rows": (C.c_int, [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
    "fn_time_logsoftmax": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_float, vp, vp]),
    "fn_time_logsoftmax_bwd": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp]),
    "fn_latent_fwd": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
    "fn_latent_bwd": (C.c_int, [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "fn_masked_prob": (C.c_int, [vp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]),
    "fn_adv_head": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, C.c_float, vp, vp, vp, vp, C.c_int, vp]),
    "fn_pairwise_reg": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, vp, C.c_float, vp, vp]),
    "fn_sumsq_ws_bytes": (C.c_size_t, [C.c_int64]),
    "fn_sumsq_f32": (C.c_int, [vp, C.c_int64, vp, vp, C.c_size_t, vp]),
    "fn_step_params": (C.c_int, [vp, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, C.c_int, vp, vp]),
    "fn_clip_adam": (C.c_int, [vp, vp, vp, vp, C.c_int64, vp, C.c_float, vp, C.c_float, C.c_float, C.c_float, vp]),
    "fn_onehot_to_index": (C.c_int, [vp, C.c_int64, C.c_int, vp, vp]),
    "fn_comm_unique_id": (C.c_int, [vp]),
    "fn_comm_init": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, vp]),
    "fn_comm_destroy": (C.c_int, [vp]),
    "fn_comm_all_reduce_f32": (C.c_int, [vp, vp, C.c_size_t, vp]),
    "fn_comm_all_gather": (C.c_int, [vp, vp, vp, C.c_size_t, vp]),
    "fn_comm_count": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "fn_comm_rank": (C.c_int, [vp, C.POINTER(C.c_int)]),
    "fn_occupy_cus": (C.c_int, [C.c_int, C.c_int, C.c_longlong, vp]),
}

_lib = None


def load():
    """Load the shared library and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libfadernets_hip.so not found at %s - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C music-fader-nets_amd/csrc`). There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.fn_version() != ABI_VERSION:
        raise RuntimeError("libfadernets_hip.so ABI version %d != %d (rebuild: make -C music-fader-nets_amd/csrc)" % (lib.fn_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(code, what):
    if code != 0:
        msg = load().fn_strerror(code)
        raise RuntimeError("%s failed: %s (code %d)" % (what, msg.decode() if msg else "?", code))
