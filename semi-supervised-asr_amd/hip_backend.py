"""ctypes binding of libasr_hip.so (C ABI declared in include/asr_hip.h).

There is NO CPU fallback: every wrapper needs device ("cuda" == HIP on ROCm)
tensors and raises if the library is absent or a tensor is on the host.
PyTorch is only the allocator / stream provider here.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libasr_hip.so")
ABI_VERSION = 8

EXPORTS = (
    "asr_abi_version", "asr_persist_scratch_bytes", "asr_gemm_f32", "asr_gemm_plan", "asr_gemm_skinny_f32", "asr_colsum_f32",
    "asr_lstm_seq_fwd", "asr_lstm_seq_fwd_persist", "asr_lstm_seq_bwd", "asr_lstm_seq_bwd_persist", "asr_lstm_seq_bwd_persist_w", "asr_lstm_bwd_persist_fuses_dw", "asr_pyramid_concat_fwd", "asr_pyramid_concat_bwd",
    "asr_pyramid_concat_fwd_seeded", "asr_pyramid_concat_bwd_seeded", "asr_rows_pack_f32", "asr_rows_unpack_fwd_f32", "asr_rows_unpack_bwd_f32", "asr_dropout_seeded_f32", "asr_relu_dropout_bwd_f32",
    "asr_dropout_mask_f32",
    "asr_dec_step_fwd", "asr_att_step_fwd", "asr_dec_seq_fwd", "asr_dec_seq_fwd_persist", "asr_dec_seq_fwd_persist_fault", "asr_dec_seq_fwd_persist_free", "asr_dec_step_bwd", "asr_dec_seq_bwd", "asr_dec_seq_bwd_persist", "asr_dec_seq_bwd_persist_free",
    "asr_lstm_pack_f32", "asr_lstm_unpack_f32", "asr_lstm_unpack2_f32", "asr_dec_prepare_f32", "asr_cell_pack_f32", "asr_cell_unpack_f32",
    "asr_lstm_pack_multi_f32", "asr_lstm_unpack_multi_f32", "asr_dec_pack_f32", "asr_colsum_parts_f32", "asr_gemm_drop_f32", "asr_gemm_side_f32", "asr_embedding_grad_f32",
    "asr_label_logprob_fwd", "asr_label_logprob_bwd", "asr_dec_feedback_fwd", "asr_dec_feedback_bwd",
    "asr_adam_clip_f32", "asr_sumsq_f32", "asr_gather_sumsq_f32",
    "asr_beam_select_f32", "asr_beam_reorder_f32", "asr_beam_backtrack",
    "asr_lm_step_f32", "asr_beam_select_lm_f32", "asr_beam_reorder_lm_f32",
    "asr_edit_distance_i32", "asr_word_edit_distance_i32",
    "asr_colsum_det_f32", "asr_gemm_det_f32", "asr_gemm_det_ws_bytes", "asr_embedding_grad_det_f32", "asr_rows_fill_grad_det_f32",
    "asr_sumsq_det_f32", "asr_gather_sumsq_det_f32", "asr_sum_det_f32", "asr_dec_step_bwd_det", "asr_dec_seq_bwd_det",
    "asr_ctc_ws_bytes", "asr_ctc_loss_fwd", "asr_ctc_loss_bwd",
    "asr_ctc_star_ws_bytes", "asr_ctc_star_loss_fwd", "asr_ctc_star_loss_bwd",
    "asr_gtc_ws_bytes", "asr_gtc_loss_fwd", "asr_gtc_loss_bwd",
    "asr_nbest_gtc_bytes", "asr_nbest_gtc_f32",
    "asr_ctc_prefix_init_f32", "asr_ctc_prefix_score_f32", "asr_beam_select_ctc_f32", "asr_ctc_prefix_advance_f32",
    "asr_ctc_align_ws_bytes", "asr_ctc_align_f32", "asr_ctc_greedy_f32",
    "asr_ctc_segment_ws_bytes", "asr_ctc_segment_f32",
    "asr_ctc_beam_ws_bytes", "asr_ctc_beam_f32", "asr_ctc_beam_lm_f32", "asr_ngram_score_f32",
    "asr_word_lm_score_f32", "asr_ctc_beam_wlm_f32",
    "asr_context_score_f32", "asr_ctc_beam_ctx_f32",
    "asr_fbank_num_frames", "asr_fbank_plan_bytes", "asr_fbank_f32", "asr_feat_cmvn_stats_f32", "asr_feat_finish_f32",
    "asr_mwer_fwd_f32", "asr_mwer_bwd_f32",
    "asr_resample_plan_bytes", "asr_resample_f32",
    "asr_reverb_f32", "asr_noise_mix_f32",
    "asr_rnnt_ws_bytes", "asr_rnnt_joint_fwd_f32", "asr_rnnt_joint_bwd_f32", "asr_rnnt_loss_fwd_f32", "asr_rnnt_loss_bwd_f32",
    "asr_rnnt_greedy_step_f32",
    "asr_transducer_align_ws_bytes", "asr_transducer_align_f32",
    "asr_transducer_beam_ws_bytes", "asr_transducer_beam_init_f32", "asr_transducer_beam_step_f32", "asr_transducer_beam_cell_f32",
    "asr_transducer_beam_backtrace_f32",
    "asr_transducer_wbeam_ws_bytes", "asr_transducer_wbeam_init_f32", "asr_transducer_wbeam_step_f32",
    "asr_transducer_wbeam_backtrace_f32",
    "asr_beam_tlm_ws_bytes", "asr_beam_tlm_init_f32", "asr_beam_select_tlm_f32", "asr_beam_backtrack_tlm",
)

_lib = None

c_i, c_i64, c_f, c_p = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p


PACK_MAX_LAYERS = 4      # ASR_PACK_MAX_LAYERS


class LstmPackJob(ctypes.Structure):
    """asr_lstm_pack_job_t"""
    _fields_ = [("H", c_i), ("I", c_i), ("ndir", c_i), ("w_ih", c_p * 2), ("w_hh", c_p * 2), ("b_ih", c_p * 2),
                ("b_hh", c_p * 2), ("w_ih_cat", c_p), ("w_hh_il", c_p), ("bias", c_p)]


class WordLmTable(ctypes.Structure):
    """asr_word_lm_t"""
    _fields_ = [("V", ctypes.c_int32), ("N", ctypes.c_int32), ("S", ctypes.c_int32), ("W", ctypes.c_int32), ("A", c_i64),
                ("space", ctypes.c_int32), ("start", ctypes.c_int32), ("empty", ctypes.c_int32), ("eos", ctypes.c_int32),
                ("unk", ctypes.c_int32), ("trie_next", c_p), ("trie_word", c_p), ("arc_off", c_p), ("arc_word", c_p),
                ("arc_logp", c_p), ("arc_next", c_p), ("bo_logp", c_p), ("bo_state", c_p), ("uni_logp", c_p), ("uni_next", c_p)]


class ContextTable(ctypes.Structure):
    """asr_context_t"""
    _fields_ = [("V", ctypes.c_int32), ("N", ctypes.c_int32), ("G", ctypes.c_int32), ("R", ctypes.c_int32), ("A", c_i64),
                ("arc_off", c_p), ("arc_tok", c_p), ("arc_next", c_p), ("drow", c_p), ("dflt", c_p), ("credit", c_p),
                ("pending", c_p), ("root", c_p)]


class GtcGraphs(ctypes.Structure):
    """asr_gtc_graphs_t"""
    _fields_ = [("V", ctypes.c_int32), ("G", ctypes.c_int32), ("max_nodes", ctypes.c_int32), ("max_arcs", ctypes.c_int32),
                ("node_off", c_p), ("lab", c_p), ("start", c_p), ("fin", c_p), ("in_ptr", c_p), ("in_src", c_p), ("in_w", c_p),
                ("out_ptr", c_p), ("out_dst", c_p), ("out_w", c_p), ("order", c_p), ("head", c_p)]


class LstmUnpackJob(ctypes.Structure):
    """asr_lstm_unpack_job_t"""
    _fields_ = [("H", c_i), ("I", c_i), ("ndir", c_i), ("dw_ih_cat", c_p), ("dw_hh_il", c_p), ("db_il", c_p),
                ("dw_ih", c_p * 2), ("dw_hh", c_p * 2), ("db", c_p * 2), ("db2", c_p * 2)]


class DecFeedback(ctypes.Structure):
    """asr_dec_feedback_t"""
    _fields_ = [("mode", c_i), ("V", c_i), ("eos", c_i), ("scaling", c_f), ("w_out", c_p), ("b_out", c_p), ("emb", c_p), ("logits", c_p),
                ("probs", c_p), ("pred", c_p), ("fed", c_p), ("tokens", c_p), ("ld_tokens", ctypes.c_int64), ("teacher", c_p)]


class DecFeedbackBwd(ctypes.Structure):
    """asr_dec_feedback_bwd_t"""
    _fields_ = [("V", c_i), ("scaling", c_f), ("w_out", c_p), ("emb", c_p), ("probs", c_p), ("dlfb", c_p)]


_DEC_DIMS = ("B", "nb", "Tp", "A", "D", "O", "E", "C", "K", "L")
_DEC_FWD_PTRS = ("P", "Q", "bo", "wcat", "bcat", "wdec", "convw", "watt", "wattT", "gvec", "w0", "xmask",
                 "X", "Xd", "gates", "cstate", "Dproj", "fconv", "S", "energy", "ws")
_DEC_BWD_PTRS = ("wcatT", "wdecT", "dws", "G", "dwext", "dwraw", "dfpart", "dP", "dgates", "dD",
                 "dcell", "dgvec_part", "dwatt_part", "dconv_part")


class DecFwd(ctypes.Structure):
    """asr_dec_fwd_t"""
    _fields_ = [(n, c_i) for n in _DEC_DIMS] + [("scaling", c_f)] + [(n, c_p) for n in _DEC_FWD_PTRS]


class Beam(ctypes.Structure):
    """asr_beam_t"""
    _fields_ = [(n, c_i) for n in ("B", "K", "V", "L", "eos")] + \
               [(n, c_p) for n in ("logits", "scores", "tok_hist", "bp_hist", "fin", "fin_score", "nfin", "done", "ndone")]


class BeamTlm(ctypes.Structure):
    """asr_beam_tlm_t"""
    _fields_ = [("kind", c_i), ("lm_states", c_i), ("lm_start", c_i), ("lm_logp", c_p), ("lm_next", c_p),
                ("word_lm", ctypes.POINTER(WordLmTable)), ("weight", c_f), ("bonus", c_f), ("lexicon_only", c_i), ("ws", c_p),
                ("ws_bytes", c_i64)]


class BeamState(ctypes.Structure):
    """asr_beam_state_t"""
    _fields_ = [(n, c_i) for n in ("D", "O", "E", "Tp")] + [("ldx", ctypes.c_int64)] + \
               [(n, c_p) for n in ("x_src", "x_dst", "c_src", "c_dst", "w_src", "w_dst", "emb")]


BEAM_KMAX, BEAM_FCAP = 16, 48          # ASR_BEAM_KMAX, ASR_BEAM_FCAP
LM_MAX_LAYERS, LM_MAX_ROWS, LM_MAX_WIDTH = 4, 512, 1024      # ASR_LM_MAX_LAYERS, ASR_LM_MAX_ROWS, ASR_LM_MAX_WIDTH


class BeamLmState(ctypes.Structure):
    """asr_beam_lm_state_t"""
    _fields_ = [("n_layers", c_i), ("H", c_i), ("in_dim", c_i * LM_MAX_LAYERS)] + \
               [(n, c_p * LM_MAX_LAYERS) for n in ("x_src", "x_dst", "c_src", "c_dst")] + [("emb", c_p)]


class CtcPrefix(ctypes.Structure):
    """asr_ctc_prefix_t"""
    _fields_ = [(n, c_i) for n in ("B", "K", "V", "Tp", "blank", "eos")] + \
               [("logits", c_p), ("ld", ctypes.c_int64), ("frame_lens", c_p), ("lse", c_p), ("state", c_p * 2), ("last", c_p * 2),
                ("psi", c_p), ("psi_prev", c_p)]


class RnntBeamArgs(ctypes.Structure):
    """asr_transducer_beam_t"""
    _fields_ = [(n, c_i) for n in ("B", "T", "J", "V", "K", "L", "E", "P")] + \
               [(n, c_p) for n in ("pe", "pp", "w_out", "b_out", "emb", "frame_lens", "h", "c", "xh")] + \
               [(n, c_i) for n in ("lm_states", "lm_start", "lm_eos")] + [("lm_alpha", c_f), ("lm_beta", c_f)] + \
               [("lm_logp", c_p), ("lm_next", c_p), ("ws", c_p), ("ws_bytes", c_i64)]


class GemmPlan(ctypes.Structure):
    """asr_gemm_plan_t"""
    _fields_ = [(n, c_i) for n in ("family", "terms", "tile", "akc", "bkc", "kt", "plain", "queue", "split_k", "tiles_m", "tiles_n",
                                   "groups")] + \
               [("grid", ctypes.c_uint * 3), ("block", ctypes.c_uint), ("pass_grid", ctypes.c_uint * 3), ("zero_pass", c_i), ("behind", c_i)]


class DecBwd(ctypes.Structure):
    """asr_dec_bwd_t"""
    _fields_ = [("f", DecFwd)] + [(n, c_p) for n in _DEC_BWD_PTRS]


def _fptr(t, off=0):
    """device pointer of float tensor t advanced by `off` elements (None stays NULL)."""
    return None if t is None else c_p(t.data_ptr() + 4 * int(off))


class DecBuffers(object):
    """Every buffer the decoder kernels read or write for B utterances and L step slots (X / Xd / G hold L + 1: slot s + 1
    is step s's output), and the two C structs over them (DecFwd / DecBwd).  Attributes carry the struct's field names.
      the constructor allocates what the kernels own: the packed weights (wcat, bcat, wattT; wcatT, wdecT), the per-step state,
            staging tensors for the inputs, and - with_bwd - the backward's scratch and its accumulators `acc` (a dict: G,
            dwext, dP, dcell, dgvec_part, dwatt_part, dconv_part), cut from ONE buffer `zbuf` that one fill zeroes;
      bind()    the per-call inputs used as they are (no staging copies), kept alive here until the next bind();
      fwd_struct / bwd_struct   the structs over all B rows (nb = B);
      accumulators(base)   `acc` laid out over another zeroed buffer (the step arena's slice) instead of zbuf."""

    _ACC = ("G", "dwext", "dP", "dcell", "dgvec_part", "dwatt_part", "dconv_part")

    def __init__(self, B, Tp, A, D, O, E, C, K, L, drop, dev, with_bwd):
        f32 = dict(device=dev, dtype=torch.float32)
        KX = D + O + E
        self.dims = dict(B=B, Tp=Tp, A=A, D=D, O=O, E=E, C=C, K=K, L=L)
        self.B, self.L, self.KX, self.scaling = B, L, KX, 2.0
        self.bo = self.wdec = self.watt = None
        self.P, self.Q, self.w0 = torch.empty(B, Tp, A, **f32), torch.empty(B, Tp, O, **f32), torch.empty(B, Tp, **f32)
        self.wcat, self.bcat, self.wattT = torch.empty(4 * D, KX, **f32), torch.empty(4 * D, **f32), torch.empty(C, A, **f32)
        self.convw, self.gvec = torch.empty(C, 2 * K + 1, **f32), torch.empty(A, **f32)
        self.X = torch.empty(L + 1, B, KX, **f32)
        self.Xd = torch.empty(L + 1, B, KX, **f32) if drop else None
        self.xmask = torch.empty(L, B, O + E, **f32) if drop else None
        self.gates, self.cstate = torch.empty(L, B, 4 * D, **f32), torch.empty(L, B, D, **f32)
        self.Dproj, self.fconv = torch.empty(L, B, A, **f32), torch.empty(L, B, C, Tp, **f32)
        self.S, self.energy, self.ws = torch.empty(L, B, Tp, A, **f32), torch.empty(L, B, Tp, **f32), torch.empty(L, B, Tp, **f32)
        self.zbuf = self.acc = None
        if with_bwd:
            ntile = (A + 63) // 64
            # everything the backward accumulates into lives in ONE buffer (16-byte aligned slices): one fill per step
            shapes = dict(G=(L + 1, B, KX), dwext=(C, B, Tp), dP=(B, Tp, A), dcell=(B, D), dgvec_part=(B, A),
                          dwatt_part=(B, A, C), dconv_part=(B, C, 2 * K + 1))
            self._acc_layout, off = [], 0
            for name in self._ACC:
                strides = torch.empty(shapes[name], device="meta").stride()
                self._acc_layout.append((name, shapes[name], strides, off))
                off += (strides[0] * shapes[name][0] + 3) // 4 * 4
            self.zbuf = torch.empty(off, **f32)
            self.acc = self.accumulators(self.zbuf)
            self.wcatT, self.wdecT = torch.empty(KX, 4 * D, **f32), torch.empty(D, A, **f32)
            self.dwraw, self.dfpart = torch.empty(B, Tp, **f32), torch.empty(ntile, B, C, Tp, **f32)
            self.dgates, self.dD = torch.empty(L, B, 4 * D, **f32), torch.empty(L, B, A, **f32)
            self.dws, self.Mf = torch.empty(L, B, Tp, **f32), torch.empty(L, B, C, Tp, **f32)
        else:
            self.wcatT = self.wdecT = None

    def bind(self, P=None, Q=None, w0=None, convw=None, gvec=None, bo=None, wdec=None, watt=None, xmask=None, scaling=None):
        """The inputs of a call (those given; the others stay as they are), made contiguous and kept alive here."""
        given = dict(P=P, Q=Q, w0=w0, bo=bo, wdec=wdec, watt=watt, xmask=xmask,
                     convw=None if convw is None else convw.reshape(self.convw.shape),
                     gvec=None if gvec is None else gvec.reshape(self.gvec.shape))
        for name, t in given.items():
            if t is not None:
                setattr(self, name, t.contiguous())
        if scaling is not None:
            self.scaling = float(scaling)

    def accumulators(self, base):
        """The backward's accumulators as views of `base`, a flat buffer of zbuf's size (one as_strided each: a slice + a
        view per accumulator cost the host 20 us more per backward, and the small configurations are host-bound)."""
        first = base.storage_offset()
        return {name: base.as_strided(shape, strides, first + off) for name, shape, strides, off in self._acc_layout}

    def fwd_struct(self):
        """asr_dec_fwd_t over all B rows."""
        return DecFwd(nb=self.B, scaling=self.scaling, **{n: _fptr(getattr(self, n)) for n in _DEC_FWD_PTRS}, **self.dims)

    def bwd_struct(self, acc=None, with_dws=True):
        """asr_dec_bwd_t over all B rows.  acc: the accumulators to use (accumulators(); None: those in zbuf);
        with_dws False: no gradient arrives through the attention weights (dws = NULL)."""
        acc, own = self.acc if acc is None else acc, self.__dict__
        ptrs = {n: _fptr(acc[n] if n in acc else own[n]) for n in _DEC_BWD_PTRS}
        if not with_dws:
            ptrs["dws"] = None
        return DecBwd(f=self.fwd_struct(), **ptrs)


def load():
    """Load the shared library once; raise loudly if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libasr_hip.so not found at %s — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). This package has no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name in EXPORTS:
        getattr(lib, name).restype = c_i
    lib.asr_persist_scratch_bytes.argtypes = [ctypes.POINTER(c_i64), ctypes.POINTER(c_i64)]
    lib.asr_gemm_f32.argtypes = [c_i, c_i, c_i64, c_i64, c_i64, c_p, c_i64, c_p, c_i64, c_p, c_i64, c_p, c_i, c_i,
                                 c_i, c_i64, c_i64, c_i64, c_i, c_i, c_p]
    lib.asr_gemm_plan.argtypes = lib.asr_gemm_f32.argtypes[:-1] + [c_i, ctypes.POINTER(GemmPlan)]
    lib.asr_gemm_skinny_f32.argtypes = [c_i64, c_i64, c_i64, c_p, c_i64, c_p, c_i64, c_p, c_i64, c_p, c_i, c_p,
                                        c_i64, c_i64, c_p]
    lib.asr_colsum_f32.argtypes = [c_i64, c_i64, c_p, c_i64, c_p, c_i, c_p]
    lib.asr_lstm_seq_fwd.argtypes = [c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]
    lib.asr_lstm_seq_fwd_persist.argtypes = [c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i, c_p]
    lib.asr_lstm_seq_bwd_persist.argtypes = [c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
                                             c_i, c_p]
    lib.asr_lstm_seq_bwd_persist_w.argtypes = lib.asr_lstm_seq_bwd_persist.argtypes
    lib.asr_lstm_bwd_persist_fuses_dw.argtypes = [c_i, c_i]
    lib.asr_lstm_seq_bwd.argtypes = [c_i, c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]
    lib.asr_rows_pack_f32.argtypes = [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_p, c_p]
    lib.asr_rows_unpack_fwd_f32.argtypes = [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_p, ctypes.c_uint64, c_f, c_p, c_p]
    lib.asr_rows_unpack_bwd_f32.argtypes = [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_i, c_p, ctypes.c_uint64, c_f, c_p, c_p, c_p, c_p]
    lib.asr_pyramid_concat_fwd.argtypes = [c_i, c_i, c_i, c_p, c_p, c_p, c_p]
    lib.asr_pyramid_concat_bwd.argtypes = [c_i, c_i, c_i, c_p, c_p, c_p, c_p]
    c_u64 = ctypes.c_uint64
    lib.asr_pyramid_concat_fwd_seeded.argtypes = [c_i, c_i, c_i, c_p, c_u64, c_f, c_p, c_p]
    lib.asr_pyramid_concat_bwd_seeded.argtypes = [c_i, c_i, c_i, c_p, c_u64, c_f, c_p, c_p]
    lib.asr_dropout_seeded_f32.argtypes = [c_i64, c_p, c_u64, c_f, c_p]
    lib.asr_relu_dropout_bwd_f32.argtypes = [c_i64, c_p, c_p, c_u64, c_f, c_p, c_p]
    lib.asr_dropout_mask_f32.argtypes = [c_i64, c_p, c_u64, c_f, c_p]
    lib.asr_dec_step_fwd.argtypes = [ctypes.POINTER(DecFwd), c_i, c_p]
    lib.asr_beam_select_f32.argtypes = [ctypes.POINTER(Beam), c_i, c_p]
    lib.asr_beam_reorder_f32.argtypes = [ctypes.POINTER(Beam), c_i, ctypes.POINTER(BeamState), c_p]
    lib.asr_beam_backtrack.argtypes = [ctypes.POINTER(Beam), c_f, c_p, c_p, c_p, c_p]
    lib.asr_lm_step_f32.argtypes = [c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_p, c_p, c_i64, c_p, c_i64, c_p]
    lib.asr_beam_select_lm_f32.argtypes = [ctypes.POINTER(Beam), c_p, c_f, c_i, c_p]
    lib.asr_beam_reorder_lm_f32.argtypes = [ctypes.POINTER(Beam), c_i, ctypes.POINTER(BeamState),
                                            ctypes.POINTER(BeamLmState), c_p]
    lib.asr_edit_distance_i32.argtypes = [c_i, c_p, c_i, c_i64, c_i, c_p, c_p, c_i64, c_p, c_p, c_i, c_p, c_i, c_p, c_p, c_p,
                                          c_p, c_p]
    lib.asr_word_edit_distance_i32.argtypes = [c_i, c_p, c_i, c_i64, c_i, c_p, c_p, c_i64, c_p, c_p, c_i, c_p, c_i, c_i, c_p, c_p,
                                               c_p, c_p, c_p]
    lib.asr_att_step_fwd.argtypes = [ctypes.POINTER(DecFwd), c_i, c_p]
    lib.asr_dec_seq_fwd.argtypes = [ctypes.POINTER(DecFwd), c_i, c_i, c_p]
    lib.asr_dec_seq_fwd_persist.argtypes = [ctypes.POINTER(DecFwd), c_p, c_p, c_p]
    lib.asr_dec_seq_fwd_persist_fault.argtypes = lib.asr_dec_seq_fwd_persist.argtypes
    lib.asr_dec_seq_fwd_persist_free.argtypes = [ctypes.POINTER(DecFwd), ctypes.POINTER(DecFeedback), c_p, c_p, c_p]
    lib.asr_dec_step_bwd.argtypes = [ctypes.POINTER(DecBwd), c_i, c_p]
    lib.asr_dec_seq_bwd.argtypes = [ctypes.POINTER(DecBwd), c_i, c_i, c_p]
    lib.asr_dec_seq_bwd_persist.argtypes = [ctypes.POINTER(DecBwd), c_p, c_p, c_p, c_p]
    lib.asr_dec_seq_bwd_persist_free.argtypes = [ctypes.POINTER(DecBwd), ctypes.POINTER(DecFeedbackBwd), c_p, c_p, c_p, c_p]
    lib.asr_adam_clip_f32.argtypes = [c_i64, c_p, c_p, c_p, c_p, c_p, c_p, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_p, c_p, c_p]
    lib.asr_sumsq_f32.argtypes = [c_i64, c_p, c_p, c_p]
    lib.asr_gather_sumsq_f32.argtypes = [c_i, ctypes.POINTER(c_p), ctypes.POINTER(c_i64), ctypes.POINTER(c_i64), c_p, c_p, c_p]
    lib.asr_label_logprob_fwd.argtypes = [c_i64, c_i, c_p, c_i64, c_p, c_p, c_f, c_p, c_p, c_f, c_p, c_p]
    lib.asr_label_logprob_bwd.argtypes = [c_i64, c_i, c_p, c_i64, c_p, c_p, c_f, c_p, c_i64, c_f, c_p, c_i64, c_p]
    lib.asr_ctc_ws_bytes.argtypes = [c_i, c_i, c_i, c_i, ctypes.POINTER(c_i64)]
    lib.asr_ctc_loss_fwd.argtypes = [c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_i64, c_p]
    lib.asr_ctc_loss_bwd.argtypes = [c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_i, c_i, c_p, c_p, c_i64, c_p, c_i64, c_p]
    lib.asr_ctc_star_ws_bytes.argtypes = [c_i, c_i, c_i, c_i, ctypes.POINTER(c_i64)]
    lib.asr_ctc_star_loss_fwd.argtypes = [c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_i, c_p, c_i, c_p, c_p, c_i64, c_p]
    lib.asr_ctc_star_loss_bwd.argtypes = [c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_i, c_p, c_i, c_p, c_p, c_i64, c_p, c_i64, c_p]
    lib.asr_gtc_ws_bytes.argtypes = [c_i, c_i, c_i, c_i, ctypes.POINTER(c_i64)]
    lib.asr_gtc_loss_fwd.argtypes = [c_i, c_i, c_i, c_p, c_i64, c_p, ctypes.POINTER(GtcGraphs), c_p, c_i, c_p, c_p, c_i64, c_p]
    lib.asr_gtc_loss_bwd.argtypes = [c_i, c_i, c_i, c_p, c_i64, c_p, ctypes.POINTER(GtcGraphs), c_p, c_i, c_p, c_p, c_i64, c_p,
                                     c_i64, c_p]
    lib.asr_nbest_gtc_bytes.argtypes = [c_i, c_i, c_i, c_i, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                        ctypes.POINTER(c_i64)]
    lib.asr_nbest_gtc_f32.argtypes = [c_i, c_i, c_i, c_i, c_p, c_p, c_p, ctypes.c_double, ctypes.POINTER(GtcGraphs), c_p, c_p,
                                      c_p, c_p, c_i64, c_p]
    lib.asr_ctc_prefix_init_f32.argtypes = [ctypes.POINTER(CtcPrefix), ctypes.POINTER(ctypes.c_int32), c_p]
    lib.asr_ctc_prefix_score_f32.argtypes = [ctypes.POINTER(CtcPrefix), ctypes.POINTER(Beam), c_i, c_p]
    lib.asr_beam_select_ctc_f32.argtypes = [ctypes.POINTER(Beam), c_p, c_f, c_p, c_p, c_f, c_i, c_p]
    lib.asr_ctc_prefix_advance_f32.argtypes = [ctypes.POINTER(CtcPrefix), ctypes.POINTER(Beam), c_i, c_i, c_i, c_p]
    lib.asr_ctc_align_ws_bytes.argtypes = [c_i, c_i, c_i, c_i, ctypes.POINTER(c_i64)]
    lib.asr_ctc_align_f32.argtypes = [c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_i64, c_p]
    lib.asr_ctc_greedy_f32.argtypes = [c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_p, c_p]
    lib.asr_ctc_segment_ws_bytes.argtypes = [c_i, c_i, c_i, c_i, ctypes.POINTER(c_i64)]
    lib.asr_ctc_segment_f32.argtypes = [c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_i, c_i, c_i, c_p, c_p, c_i,
                                        c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i64, c_p]
    lib.asr_ctc_beam_ws_bytes.argtypes = [c_i, c_i, c_i, c_i, ctypes.POINTER(c_i64)]
    lib.asr_ctc_beam_f32.argtypes = [c_i, c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_p, c_p, c_p]
    lib.asr_ctc_beam_lm_f32.argtypes = [c_i, c_i, c_i, c_i, c_p, c_i64, c_p, c_i, c_p, c_p, c_i, c_i, c_f, c_f, c_p, c_p, c_p, c_p, c_p,
                                        c_p, c_p]
    lib.asr_ngram_score_f32.argtypes = [c_i, c_i, c_i, c_i, c_p, c_p, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_p]
    lib.asr_word_lm_score_f32.argtypes = [c_i, c_i, ctypes.POINTER(WordLmTable), c_i, c_p, c_i64, c_p, c_p, c_p, c_p, c_p]
    lib.asr_context_score_f32.argtypes = [c_i, c_i, ctypes.POINTER(ContextTable), c_p, c_p, c_i64, c_p, c_p, c_p, c_p]
    lib.asr_ctc_beam_ctx_f32.argtypes = [c_i, c_i, c_i, c_i, c_p, c_i64, c_p, ctypes.POINTER(ContextTable), c_p, c_f, c_i, c_p, c_p,
                                         c_i, c_i, c_f, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]
    lib.asr_ctc_beam_wlm_f32.argtypes = [c_i, c_i, c_i, c_i, c_p, c_i64, c_p, ctypes.POINTER(WordLmTable), c_f, c_f, c_i, c_i, c_p, c_p,
                                         c_p, c_p, c_p, c_p, c_p, c_p]
    lib.asr_fbank_num_frames.argtypes = [c_i64, c_i, c_i, ctypes.POINTER(c_i64)]
    lib.asr_fbank_plan_bytes.argtypes = [c_i, ctypes.POINTER(c_i64)]
    lib.asr_fbank_f32.argtypes = [c_i, c_i, c_p, c_i, c_p, c_i, c_i, c_i, c_i, c_f, c_i, c_p, c_p, c_i64, c_i64, c_p]
    lib.asr_feat_cmvn_stats_f32.argtypes = [c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p]
    lib.asr_feat_finish_f32.argtypes = [c_i, c_i, c_i, c_i, c_p, c_i64, c_p, c_i, c_p, c_p, c_i, c_i, c_p, c_p]
    lib.asr_resample_plan_bytes.argtypes = [c_i, c_p, ctypes.POINTER(c_i64)]
    lib.asr_resample_f32.argtypes = [c_i, c_i64, c_p, c_i, c_i64, c_p, c_p, c_p, c_i, c_p, c_p, c_i64, c_p, c_i64, c_p]
    lib.asr_reverb_f32.argtypes = [c_i, c_i64, c_p, c_i, c_i64, c_p, c_p, c_i, c_p, c_p, c_p, c_i64, c_p, c_i64, c_p]
    lib.asr_noise_mix_f32.argtypes = [c_i, c_i64, c_p, c_i, c_i64, c_p, c_p, c_p, c_p, c_i, c_p, c_p, c_p, c_i64, c_p, c_i64, c_p,
                                      c_i64, c_p, c_p]
    lib.asr_rnnt_ws_bytes.argtypes = [c_i, c_i, c_i, c_i, c_i, ctypes.POINTER(c_i64)]
    lib.asr_rnnt_joint_fwd_f32.argtypes = [c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p]
    lib.asr_rnnt_joint_bwd_f32.argtypes = [c_i, c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]
    lib.asr_rnnt_loss_fwd_f32.argtypes = [c_i, c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_p, c_p, c_i64, c_p]
    lib.asr_rnnt_loss_bwd_f32.argtypes = [c_i, c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_p, c_p, c_i64, c_p, c_i64, c_p]
    lib.asr_rnnt_greedy_step_f32.argtypes = [c_i] * 6 + [c_p] * 13
    lib.asr_transducer_align_ws_bytes.argtypes = [c_i, c_i, c_i, c_i, ctypes.POINTER(c_i64)]
    lib.asr_transducer_align_f32.argtypes = [c_i, c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i64, c_p]
    lib.asr_transducer_beam_ws_bytes.argtypes = [c_i] * 8 + [ctypes.POINTER(c_i64)]
    lib.asr_transducer_beam_init_f32.argtypes = [ctypes.POINTER(RnntBeamArgs), c_i, c_p]
    lib.asr_transducer_beam_step_f32.argtypes = [ctypes.POINTER(RnntBeamArgs), c_i, c_p]
    lib.asr_transducer_beam_cell_f32.argtypes = [ctypes.POINTER(RnntBeamArgs), c_p, c_p, c_p, c_p]
    lib.asr_transducer_beam_backtrace_f32.argtypes = [ctypes.POINTER(RnntBeamArgs), c_p, c_p, c_p, c_p, c_p, c_p]
    wbeam = [ctypes.POINTER(RnntBeamArgs), ctypes.POINTER(WordLmTable), c_f, c_f, c_i, c_i, c_p, c_i64]
    lib.asr_transducer_wbeam_ws_bytes.argtypes = [c_i, c_i, ctypes.POINTER(c_i64)]
    lib.asr_transducer_wbeam_init_f32.argtypes = wbeam + [c_i, c_p]
    lib.asr_transducer_wbeam_step_f32.argtypes = wbeam + [c_i, c_p]
    lib.asr_transducer_wbeam_backtrace_f32.argtypes = wbeam + [c_p] * 7
    lib.asr_beam_tlm_ws_bytes.argtypes = [c_i, c_i, ctypes.POINTER(c_i64)]
    lib.asr_beam_tlm_init_f32.argtypes = [ctypes.POINTER(Beam), ctypes.POINTER(BeamTlm), c_p]
    lib.asr_beam_select_tlm_f32.argtypes = [ctypes.POINTER(Beam), ctypes.POINTER(BeamTlm), c_p, c_f, c_p, c_p, c_f, c_i, c_p]
    lib.asr_beam_backtrack_tlm.argtypes = [ctypes.POINTER(Beam), ctypes.POINTER(BeamTlm), c_f] + [c_p] * 7
    lib.asr_mwer_fwd_f32.argtypes = [c_i, c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_f, c_p, c_p, c_p, c_p, c_p, c_p, c_i64, c_p]
    lib.asr_mwer_bwd_f32.argtypes = [c_i, c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_p, c_f, c_p, c_i64, c_p]
    lib.asr_dec_feedback_fwd.argtypes = [c_i, c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_p, c_p, c_i, c_f, c_p, c_i64,
                                         c_p, c_p, c_p, c_p, c_p, c_i64, c_p]
    lib.asr_dec_feedback_bwd.argtypes = [c_i, c_i, c_i, c_i, c_p, c_p, c_i64, c_p, c_p, c_p, c_f, c_p, c_p]
    pp = ctypes.POINTER(c_p)
    lib.asr_lstm_pack_f32.argtypes = [c_i, c_i, c_i, pp, pp, pp, pp, c_p, c_p, c_p, c_p]
    lib.asr_lstm_unpack_f32.argtypes = [c_i, c_i, c_i, c_p, c_p, c_p, pp, pp, pp, c_p]
    lib.asr_lstm_unpack2_f32.argtypes = [c_i, c_i, c_i, c_p, c_p, c_p, pp, pp, pp, pp, c_p]
    lib.asr_dec_prepare_f32.argtypes = [c_i, c_i, c_i, c_i, c_i, c_p, c_i64, c_p, c_p, c_p, c_p, c_p, c_p]
    lib.asr_cell_pack_f32.argtypes = [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]
    lib.asr_cell_unpack_f32.argtypes = [c_i, c_i, c_i, c_p, c_p, c_p, c_p, c_p, c_p, c_p]
    lib.asr_lstm_pack_multi_f32.argtypes = [c_i, ctypes.POINTER(LstmPackJob), c_p]
    lib.asr_lstm_unpack_multi_f32.argtypes = [c_i, ctypes.POINTER(LstmUnpackJob), c_p]
    lib.asr_dec_pack_f32.argtypes = [c_i, c_i, c_i, c_i, c_i] + [c_p] * 12
    lib.asr_colsum_parts_f32.argtypes = [c_i, c_i, pp, ctypes.POINTER(ctypes.c_int32), pp, c_p]
    lib.asr_embedding_grad_f32.argtypes = [c_i64, c_i, c_i, c_p, c_p, c_i64, c_p, c_p]
    lib.asr_gemm_drop_f32.argtypes = [c_i, c_i, c_i64, c_i64, c_i64, c_p, c_i64, c_p, c_i64, c_p, c_i64, c_p, c_i, c_i, c_i,
                                      ctypes.c_uint64, c_f, c_p]
    lib.asr_gemm_side_f32.argtypes = [c_i, c_i, c_i64, c_i64, c_i64, c_p, c_i64, c_p, c_i64, c_p, c_i64, c_i, c_i64, c_i64, c_i64,
                                      c_i, ctypes.c_uint, c_p, c_p]
    lib.asr_colsum_det_f32.argtypes = [c_i64, c_i64, c_p, c_i64, c_p, c_i, c_p, c_i64, c_p]
    lib.asr_gemm_det_f32.argtypes = lib.asr_gemm_f32.argtypes[:-1] + [c_p, c_i64, c_p]
    lib.asr_gemm_det_ws_bytes.argtypes = lib.asr_gemm_f32.argtypes[:-1] + [ctypes.POINTER(c_i64), ctypes.POINTER(c_i),
                                                                            ctypes.POINTER(c_i64)]
    lib.asr_embedding_grad_det_f32.argtypes = lib.asr_embedding_grad_f32.argtypes
    lib.asr_rows_fill_grad_det_f32.argtypes = [c_i, c_i, c_i, c_p, c_p, c_p, ctypes.c_uint64, c_f, c_p, c_p, c_p, c_i64, c_p]
    lib.asr_sumsq_det_f32.argtypes = [c_i64, c_p, c_p, c_p, c_i64, c_p]
    lib.asr_gather_sumsq_det_f32.argtypes = [c_i, ctypes.POINTER(c_p), ctypes.POINTER(c_i64), ctypes.POINTER(c_i64), c_p, c_p, c_p,
                                             c_i64, c_p]
    lib.asr_sum_det_f32.argtypes = [c_i64, c_p, c_f, c_p, c_p]
    lib.asr_dec_step_bwd_det.argtypes = lib.asr_dec_step_bwd.argtypes
    lib.asr_dec_seq_bwd_det.argtypes = lib.asr_dec_seq_bwd.argtypes
    if lib.asr_abi_version() != ABI_VERSION:
        raise RuntimeError("libasr_hip.so ABI %d != expected %d" % (lib.asr_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


# Product arithmetic of the MFMA kernels (include/asr_hip.h: ASR_ARITH_*): an explicit argument of every C-ABI call.
# This module only holds the host code's DEFAULT for calls that do not name one: bf16x6 (three-term split, six products:
# fp32-equivalent), overridable with ASR_ARITH=f32|bf16x6|bf16x3 or `with hb.arith("f32"):`.
ARITH_F32, ARITH_BF16X6, ARITH_BF16X3 = 0, 1, 2
GEMM_TILE_NARROW, GEMM_TILE_WIDE, LSTM_BWD_GATHER, GEMM_TILE_SP, GEMM_TILE_SMALL = 0x100, 0x200, 0x400, 0x800, 0x1000
DEBUG_FAULT = 0x10000        # ASR_DEBUG_FAULT: the persistent LSTM forward launch aborts by itself (tests of the abort path)
# tests of the abort path: True routes the next teacher-forced persistent decoder launch to asr_dec_seq_fwd_persist_fault
DEC_FAULT = [False]
ARITH_NAMES = {"f32": ARITH_F32, "bf16x6": ARITH_BF16X6, "bf16x3": ARITH_BF16X3}
ARITH_LABEL = {ARITH_F32: "f32", ARITH_BF16X6: "bf16x6", ARITH_BF16X3: "bf16x3"}


def _arith_code(a):
    if isinstance(a, str):
        code = 0
        for part in a.lower().split("+"):
            code |= {"narrow": GEMM_TILE_NARROW, "wide": GEMM_TILE_WIDE, "gather": LSTM_BWD_GATHER, "sp": GEMM_TILE_SP,
                     "small": GEMM_TILE_SMALL, "fault": DEBUG_FAULT}.get(part, 0) or \
                    ARITH_NAMES[part]
        return code
    return int(a)


ARITH = [_arith_code(os.environ.get("ASR_ARITH", "bf16x6"))]


def current_arith():
    return ARITH[0]


def arith_name(a=None):
    return ARITH_LABEL[(ARITH[0] if a is None else _arith_code(a)) & 0xff]


class arith(object):
    """Context manager: host-side default arithmetic for the calls inside (name, code, or name+flag: "bf16x3+wide")."""

    def __init__(self, a):
        self.code = _arith_code(a)

    def __enter__(self):
        self.old = ARITH[0]
        ARITH[0] = self.code
        return self

    def __exit__(self, *exc):
        ARITH[0] = self.old
        return False


# Deterministic mode (include/asr_hip.h "Deterministic mode"): with the cell set, every wrapper below whose
# default entry adds fp32 partial sums with atomics calls the ordered entry of csrc/reduce_det.hip instead, the persistent
# LSTM backward leaves dW_hh and the bias gradient to the caller's (ordered) product and column sum, the decoder backward
# runs on the per-step kernels, and the side stream is not used (ops._SideStream.usable).  Off by default; env
# ASR_DETERMINISTIC=1, config key `deterministic` (solver.py), `with hb.deterministic():`.  The library has no such state:
# the mode is WHICH entry the host code calls.
DETERMINISTIC = [os.environ.get("ASR_DETERMINISTIC", "0") == "1"]


def is_deterministic():
    return DETERMINISTIC[0]


class deterministic(object):
    """Context manager: deterministic mode on (or off) for the calls inside."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        self.old = DETERMINISTIC[0]
        DETERMINISTIC[0] = self.on
        return self

    def __exit__(self, *exc):
        DETERMINISTIC[0] = self.old
        return False


_det_ws_cache = {}


def det_workspace(device, nbytes):
    """Scratch of the ordered reductions: one buffer per (device, stream) - calls on one stream are ordered, so they share it
    - grown to the largest request so far and kept for the life of the process (tens of MB at cfg-2: the slabs of the widest
    weight-gradient product).  HOST-SIDE STATE of this module, like the persistent kernels' scratch pair: the library itself
    stays stateless, the buffer is an argument of every call.  Not the step arena: that is zeroed at every step, and these
    bytes are written before they are read.  -> (pointer, bytes); (None, 0) for nbytes <= 0."""
    if nbytes <= 0:
        return None, 0
    key = (_scratch_key(device), _raw_stream(_raw_device()) if _raw_stream is not None and _raw_device is not None
           else torch.cuda.current_stream().cuda_stream)
    buf = _det_ws_cache.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = _det_ws_cache[key] = torch.empty((int(nbytes) + 3) // 4 + 1024, device=device, dtype=torch.float32)
    return c_p(buf.data_ptr()), buf.numel() * 4


def _dev(t, name="tensor"):
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU: the HIP path has no CPU fallback" % name)
    if t.dtype not in (torch.float32, torch.int32):
        raise RuntimeError("%s must be float32/int32, got %s" % (name, t.dtype))
    return t


def ptr(t):
    return None if t is None else c_p(_dev(t).data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def stream():
    """The current HIP stream of the current device as the C ABI takes it.  Asked ~85 times per train step (once per launch):
    the raw handle straight from torch's C layer (0.3 us) instead of a torch.cuda.Stream object per call (2.3 us each - 0.2
    ms of a cfg-1 step whose 2.4 ms ARE its host time)."""
    if _raw_stream is not None and _raw_device is not None:
        return c_p(_raw_stream(_raw_device()))
    return c_p(torch.cuda.current_stream().cuda_stream)


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed with code %d (negative: ASR_E_*; positive: hipError_t)" % (what, rc))


def _rowmajor(t):
    """2-D view with unit column stride -> (tensor, leading dimension)."""
    assert t.dim() == 2 and (t.stride(1) == 1 or t.shape[1] == 1), "need row-major 2-D view"
    return t, (t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1))


C_ZEROED = 0x2000          # ASR_GEMM_C_ZEROED


def gemm(A, B, trans_a=False, trans_b=False, bias=None, relu=False, out=None, accumulate=False, split_k=None, arith=None,
         drop=None, out_zeroed=False):
    """out[M,N] = op(A) op(B) (+bias)(relu)(+out).  A, B, out are 2-D row-major views (row stride free).
    split_k None: the library chooses (asr_gemm_f32 with split_k = 0); 1: unsplit, run-to-run deterministic.
    drop (SeededMask): the seeded dropout mask over out's element index behind the epilogue (asr_gemm_drop_f32).
    out_zeroed: `out` holds zeros (a slice of the step's arena): a product split over K needs no zero pass of its own."""
    A, lda = _rowmajor(_dev(A, "A"))
    B, ldb = _rowmajor(_dev(B, "B"))
    M, K = (A.shape[1], A.shape[0]) if trans_a else A.shape
    K2, N = (B.shape[1], B.shape[0]) if trans_b else B.shape
    assert K == K2, "inner dimensions differ: %d vs %d" % (K, K2)
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    out, ldc = _rowmajor(out)
    assert out.shape == (M, N)
    code = (ARITH[0] if arith is None else _arith_code(arith)) | (C_ZEROED if out_zeroed else 0)
    if drop is not None:
        assert not accumulate and ldc == N
        if DETERMINISTIC[0]:
            split_k = 1                # (the dropout epilogue sits on forward products, whose K is small: unsplit)
        check(load().asr_gemm_drop_f32(int(trans_a), int(trans_b), M, N, K, ptr(A), lda, ptr(B), ldb, ptr(out), ldc,
                                       ptr(bias), int(relu), 0 if split_k is None else int(split_k), code, drop.seed,
                                       float(drop.p), stream()), "asr_gemm_drop_f32")
        return out
    if DETERMINISTIC[0] and split_k != 1:
        return _gemm_det((int(trans_a), int(trans_b), M, N, K, ptr(A), lda, ptr(B), ldb, ptr(out), ldc, ptr(bias), int(relu),
                          int(accumulate), 1, 0, 0, 0, 0 if split_k is None else int(split_k), code), out)
    check(load().asr_gemm_f32(int(trans_a), int(trans_b), M, N, K, ptr(A), lda, ptr(B), ldb, ptr(out), ldc,
                              ptr(bias), int(relu), int(accumulate), 1, 0, 0, 0, 0 if split_k is None else int(split_k),
                              code, stream()), "asr_gemm_f32")
    return out


def gemm_batched(A, B, out, trans_a, trans_b, M, N, K, lda, ldb, ldc, batch, sA, sB, sC, accumulate=False, arith=None,
                 split_k=None, a_off=0, b_off=0):
    """Raw batched form (pointer + strides in elements; strides may be negative); tensors only provide the base pointers
    (a_off / b_off: element offsets of the first operand elements inside A / B)."""
    args = (int(trans_a), int(trans_b), M, N, K, _off(A, a_off), lda, _off(B, b_off), ldb, ptr(out), ldc,
            None, 0, int(accumulate), batch, sA, sB, sC, 0 if split_k is None else int(split_k),
            ARITH[0] if arith is None else _arith_code(arith))
    if DETERMINISTIC[0] and split_k != 1:
        return _gemm_det(args, out)
    check(load().asr_gemm_f32(*args, stream()), "asr_gemm_f32(batched)")
    return out


def _gemm_det(args, out):
    """asr_gemm_det_f32 on the argument tuple of asr_gemm_f32 (without the stream): the K split as ordered slabs."""
    lib = load()
    need, S, kr = c_i64(0), c_i(0), c_i64(0)
    check(lib.asr_gemm_det_ws_bytes(*args, ctypes.byref(need), ctypes.byref(S), ctypes.byref(kr)), "asr_gemm_det_ws_bytes")
    ws, nbytes = det_workspace(out.device, need.value)
    check(lib.asr_gemm_det_f32(*args, ws, nbytes, stream()), "asr_gemm_det_f32")
    return out


def gemm_det(A, B, trans_a=False, trans_b=False, bias=None, relu=False, out=None, accumulate=False, split=None, arith=None):
    """gemm() through asr_gemm_det_f32 whatever the mode; split: the number of K ranges asked for (None: the library's rule)."""
    with deterministic(True):
        return gemm(A, B, trans_a, trans_b, bias, relu, out, accumulate, 0 if split is None else int(split), arith)


def gemm_det_split(M, N, K, trans_a=False, trans_b=False, split=None, batch=1, arith=None, lda=None, ldb=None, ldc=None,
                   accumulate=False, bias=False, relu=False):
    """asr_gemm_det_ws_bytes on plain integers (no tensors, no GPU) -> dict(rc, bytes, split, k_range): the workspace
    asr_gemm_det_f32 needs, the K ranges it forms and their length; rc != 0: the refusal, the rest missing."""
    lda, ldb, ldc = lda or (M if trans_a else K), ldb or (K if trans_b else N), ldc or N
    need, S, kr = c_i64(0), c_i(0), c_i64(0)
    rc = load().asr_gemm_det_ws_bytes(int(trans_a), int(trans_b), M, N, K, 64, lda, 64, ldb, 64, ldc, 64 if bias else None,
                                      int(relu), int(accumulate), batch, 0, 0, 0, 0 if split is None else int(split),
                                      ARITH[0] if arith is None else _arith_code(arith), ctypes.byref(need), ctypes.byref(S),
                                      ctypes.byref(kr))
    return dict(rc=rc) if rc != 0 else dict(rc=0, bytes=need.value, split=S.value, k_range=kr.value)


GEMM_FAMILIES = ("f32", "bf3", "bfw", "bfs", "bfk")          # ASR_GEMM_FAMILY_*


def gemm_plan(M, N, K, trans_a=False, trans_b=False, lda=None, ldb=None, ldc=None, batch=1, sA=0, sB=0, sC=0, bias=False,
              relu=False, accumulate=False, drop=False, split_k=None, arith=None, misaligned=0):
    """What gemm() / gemm_batched() would launch for these sizes (asr_gemm_plan; plain integers, no tensors, no GPU): the
    fields of asr_gemm_plan_t, `rc` (the code the call would return before launching; the other fields are missing when
    it is not 0), `kernel` (the product kernel in the short form of tools/isa_guard.py) and `launches` (every launch in
    order as (kernel, grid in workgroups, threads per workgroup): zero pass, product, pass behind).
    Leading dimensions default to dense, pointers to 16-byte aligned (misaligned: bit 0 / 1 / 2 = A / B / C is not)."""
    lda, ldb, ldc = lda or (M if trans_a else K), ldb or (K if trans_b else N), ldc or N
    code = ARITH[0] if arith is None else _arith_code(arith)
    p = GemmPlan()
    rc = load().asr_gemm_plan(int(trans_a), int(trans_b), M, N, K, 64 + 4 * (misaligned & 1), lda, 64 + 4 * (misaligned >> 1 & 1), ldb,
                              64 + 4 * (misaligned >> 2 & 1), ldc, 64 if bias else None, int(relu), int(accumulate), batch, sA, sB, sC,
                              0 if split_k is None else int(split_k), code, int(drop), ctypes.byref(p))
    if rc != 0:
        return dict(rc=rc, launches=[])
    d = {n: (list(v) if hasattr(v, "__len__") else v) for n, v in ((f[0], getattr(p, f[0])) for f in GemmPlan._fields_)}
    tf = lambda *v: ",".join(("true" if x else "false") if isinstance(x, bool) else str(x) for x in v)
    lay = (bool(p.akc), bool(p.bkc))
    d["family"] = fam = GEMM_FAMILIES[p.family]
    d["kernel"] = {"f32": "gemm_f32_kernel<%s>" % tf(*lay), "bf3": "gemm_bf3_kernel<%s>" % tf(*lay, p.terms, p.tile, bool(p.queue)),
                   "bfw": "gemm_bf%dw_kernel<%s>" % (6 if p.terms == 3 else 3, tf(*lay)),
                   "bfs": "gemm_bfs_kernel<%s>" % tf(*lay, p.terms, bool(p.kt)), "bfk": "gemm_bfk_kernel<%s>" % tf(p.terms, 5, bool(p.plain))}[fam]
    d["behind"] = [s for b, s in ((1, "epilogue"), (2, "dropout")) if p.behind & b]
    d["launches"] = ([("zero_rows_kernel", d["pass_grid"], 256)] if p.zero_pass else []) + [(d["kernel"], d["grid"], p.block)] + \
                    ([("bias_act_kernel", d["pass_grid"], 256)] if p.behind else [])
    d["rc"] = 0
    return d


def gemm_side(A, B, out, queue, xcd_mask, trans_a=False, trans_b=False, arith=None):
    """out[M,N] += op(A) op(B) on the XCDs of `xcd_mask` only, by workgroups that fit beside a persistent kernel
    (asr_gemm_side_f32); `queue`: a zeroed int32 / float32 word (tensor), consumed.  False when the arithmetic has no such
    kernel (the fp32-input MFMA): the caller runs gemm() instead."""
    code = ARITH[0] if arith is None else _arith_code(arith)
    if (code & 0xff) == ARITH_F32:
        return False
    A, lda = _rowmajor(_dev(A, "A"))
    B, ldb = _rowmajor(_dev(B, "B"))
    M, K = (A.shape[1], A.shape[0]) if trans_a else A.shape
    K2, N = (B.shape[1], B.shape[0]) if trans_b else B.shape
    assert K == K2 and out.shape == (M, N)
    out, ldc = _rowmajor(out)
    check(load().asr_gemm_side_f32(int(trans_a), int(trans_b), M, N, K, ptr(A), lda, ptr(B), ldb, ptr(out), ldc, 1, 0, 0, 0,
                                   code, int(xcd_mask) & 0xff, c_p(queue.data_ptr()), stream()), "asr_gemm_side_f32")
    return True


def gemm_side_batched(A, B, out, queue, xcd_mask, trans_a, trans_b, M, N, K, lda, ldb, ldc, batch, sA, sB, sC, arith=None,
                      a_off=0, b_off=0):
    """The raw batched form of gemm_side (as gemm_batched)."""
    code = ARITH[0] if arith is None else _arith_code(arith)
    if (code & 0xff) == ARITH_F32:
        return False
    check(load().asr_gemm_side_f32(int(trans_a), int(trans_b), M, N, K, _off(A, a_off), lda, _off(B, b_off), ldb, ptr(out), ldc,
                                   batch, sA, sB, sC, code, int(xcd_mask) & 0xff, c_p(queue.data_ptr()), stream()),
          "asr_gemm_side_f32(batched)")
    return True


def gemm_skinny(A, Bt, bias=None, out=None, accumulate=False):
    """out[M,N] (+)= A[M,K] Bt[N,K]^T (+bias) for small M (the sequential chains)."""
    A, lda = _rowmajor(_dev(A, "A"))
    Bt, ldb = _rowmajor(_dev(Bt, "Bt"))
    M, K = A.shape
    N = Bt.shape[0]
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    out, ldc = _rowmajor(out)
    check(load().asr_gemm_skinny_f32(M, N, K, ptr(A), lda, ptr(Bt), ldb, ptr(out), ldc, ptr(bias), int(accumulate),
                                     None, 0, 0, stream()), "asr_gemm_skinny_f32")
    return out


class BeamSearch:
    """The device state of one beam search (asr_beam_t): B utterances, beam width K, vocabulary V, at most L steps.
    select / reorder / backtrack enqueue the three beam kernels (csrc/beam.hip) on the current stream; `ndone` is the
    device word the host polls."""

    def __init__(self, B, K, V, L, eos, device):
        if not 1 <= K <= BEAM_KMAX:
            raise ValueError("beam width %d outside 1..%d" % (K, BEAM_KMAX))
        i32 = dict(dtype=torch.int32, device=device)
        self.B, self.K, self.V, self.L, self.eos = B, K, V, L, eos
        self.scores = torch.full((B, K), float("-inf"), dtype=torch.float32, device=device)
        self.scores[:, 0] = 0.0
        self.tok_hist = torch.empty(L, B, K, **i32)
        self.bp_hist = torch.empty(L, B, K, **i32)
        self.fin = torch.empty(B, BEAM_FCAP, 4, **i32)
        self.fin_score = torch.empty(B, BEAM_FCAP, dtype=torch.float32, device=device)
        counters = torch.zeros(2 * B + 1, **i32)                 # nfin | done | ndone: one fill
        self.nfin, self.done, self.ndone = counters[:B], counters[B:2 * B], counters[2 * B:]
        self._counters = counters
        self.struct = Beam(B=B, K=K, V=V, L=L, eos=eos, logits=None, scores=ptr(self.scores),
                           tok_hist=ptr(self.tok_hist), bp_hist=ptr(self.bp_hist), fin=ptr(self.fin),
                           fin_score=ptr(self.fin_score), nfin=ptr(self.nfin), done=ptr(self.done), ndone=ptr(self.ndone))

    def _step(self, logits, lm_logits=None, ctc=None):
        """What every select shares: logits [B*K, V] contiguous, lm_logits like them, ctc.psi of their shape -> the struct with
        the step's logits."""
        assert logits.is_contiguous() and tuple(logits.shape) == (self.B * self.K, self.V)
        assert lm_logits is None or (lm_logits.is_contiguous() and lm_logits.shape == logits.shape)
        assert ctc is None or tuple(ctc.psi.shape) == (self.B * self.K, self.V)
        self.struct.logits = ptr(logits)
        return ctypes.byref(self.struct)

    def select(self, logits, t):
        """logits [B*K, V] (contiguous) of step t -> tokens, backpointers, scores, finished list, done flags."""
        check(load().asr_beam_select_f32(self._step(logits), int(t), stream()), "asr_beam_select_f32")

    def select_lm(self, logits, lm_logits, lm_weight, t):
        """select() on score + log_softmax(logits) + lm_weight * log_softmax(lm_logits) (shallow fusion);
        lm_logits [B*K, V] like logits."""
        check(load().asr_beam_select_lm_f32(self._step(logits, lm_logits), ptr(lm_logits), float(lm_weight), int(t), stream()),
              "asr_beam_select_lm_f32")

    def select_ctc(self, logits, ctc, ctc_weight, t, lm_logits=None, lm_weight=0.0):
        """select() / select_lm() (lm_logits given) with the CTC prefix score of `ctc` (CtcPrefixState, after its score()):
        score + (1 - ctc_weight) * logp + ctc_weight * (psi - psi_prev) (+ lm_weight * logp_lm) - DESIGN 4.15.
        ctc_weight = 0 launches the plain / LM select."""
        check(load().asr_beam_select_ctc_f32(self._step(logits, lm_logits, ctc), ptr(lm_logits), float(lm_weight), ptr(ctc.psi),
                                             ptr(ctc.psi_prev), float(ctc_weight), int(t), stream()), "asr_beam_select_ctc_f32")

    @staticmethod
    def _state(x_src, x_dst, c_src, c_dst, w_src, w_dst, emb, D, O):
        assert x_dst.stride(0) == x_src.stride(0) and emb.is_contiguous()
        return BeamState(D=D, O=O, E=emb.shape[1], Tp=w_src.shape[1], ldx=x_src.stride(0), x_src=ptr(x_src),
                         x_dst=ptr(x_dst), c_src=ptr(c_src), c_dst=ptr(c_dst), w_src=ptr(w_src), w_dst=ptr(w_dst),
                         emb=ptr(emb))

    def reorder(self, t, x_src, x_dst, c_src, c_dst, w_src, w_dst, emb, D, O):
        """Gather the step-t state of every live beam's predecessor: x rows [B*K, ldx] (z | ctx | embedding columns),
        cell state [B*K, D], attention weights [B*K, Tp]; the new tokens' embedding rows into x_dst[:, D+O:]."""
        st = self._state(x_src, x_dst, c_src, c_dst, w_src, w_dst, emb, D, O)
        check(load().asr_beam_reorder_f32(ctypes.byref(self.struct), int(t), ctypes.byref(st), stream()),
              "asr_beam_reorder_f32")

    def reorder_lm(self, t, lm_state, dec=None):
        """The LM state of every live beam's predecessor (lm_state: LmStepState - every layer's h and c from the output
        slot into the input slot, the new tokens' LM embedding into layer 0's x part) and, in the same launch, the
        decoder's gather (dec: the arguments of reorder() after t; None: the LM state alone)."""
        st = self._state(*dec) if dec is not None else None
        check(load().asr_beam_reorder_lm_f32(ctypes.byref(self.struct), int(t), ctypes.byref(st) if st is not None else None,
                                             ctypes.byref(lm_state.reorder_struct()), stream()), "asr_beam_reorder_lm_f32")

    def _hyps(self):
        """A backtrack's outputs: tokens [B, K, L] int32, scores [B, K] fp32, lengths [B, K] int32."""
        dev = self.scores.device
        return (torch.empty(self.B, self.K, self.L, dtype=torch.int32, device=dev),
                torch.empty(self.B, self.K, dtype=torch.float32, device=dev),
                torch.empty(self.B, self.K, dtype=torch.int32, device=dev))

    def backtrack(self, length_penalty=0.0):
        """-> tokens [B, K, L] int32 (ranked, <EOS>-padded), scores [B, K] (score / len**length_penalty), lengths [B, K]."""
        tokens, scores, lengths = self._hyps()
        check(load().asr_beam_backtrack(ctypes.byref(self.struct), float(length_penalty), ptr(tokens), ptr(scores),
                                        ptr(lengths), stream()), "asr_beam_backtrack")
        return tokens, scores, lengths


BEAM_TLM_NGRAM, BEAM_TLM_WORD = 1, 2     # ASR_BEAM_TLM_NGRAM, ASR_BEAM_TLM_WORD


def beam_tlm_ws_bytes(B, K):
    """asr_beam_tlm_ws_bytes on plain integers (no tensors, no GPU) -> the EXTRA workspace bytes of an attention beam search with
    an n-gram or word LM inside: 4 (4 round64(B K) + 3 round64(B BEAM_FCAP)); UnsupportedShape for a beam outside
    1 .. BEAM_KMAX."""
    need = c_i64(0)
    rc = load().asr_beam_tlm_ws_bytes(int(B), int(K), ctypes.byref(need))
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("beam_tlm: B %d, beam %d (beam 1 .. %d)" % (B, K, BEAM_KMAX))
    check(rc, "asr_beam_tlm_ws_bytes")
    return need.value


class BeamTableLm:
    """The n-gram automaton (ngram: the table on the device) or the lexicon and word LM (word_lm: word_lm.WordTable after
    .to(device)) inside a BeamSearch (asr_beam_tlm_t, the asr_beam_*_tlm entries of csrc/beam.hip): candidates rank
    by (base + weight lm) + bonus len (word LM: n_words), search.scores keeps base.  ws: the extra workspace (float32 or
    int32, at least beam_tlm_ws_bytes bytes), the caller's; it holds the LM position of every beam row and the parts of the
    finished entries.  init() before step 0, select() in place of the search's select / select_lm / select_ctc, backtrack()
    in place of its backtrack: one launch each."""

    def __init__(self, search, ws, ngram=None, word_lm=None, weight=0.0, bonus=0.0, lexicon_only=False):
        if (ngram is None) == (word_lm is None):
            raise ValueError("beam_tlm: one of ngram and word_lm")
        self.search = search
        t = BeamTlm()
        if ngram is not None:
            logp, nxt, S = _ngram_table(ngram, search.V, "beam_tlm")
            t.kind, t.lm_states, t.lm_start, t.lm_logp, t.lm_next = BEAM_TLM_NGRAM, S, int(ngram.start), ptr(logp), ptr(nxt)
            self._keep = (ngram, logp, nxt, ws)
        else:
            if word_lm.V != search.V:
                raise UnsupportedShape("beam_tlm: the word LM spells in %d tokens, the search is over %d" % (word_lm.V, search.V))
            self._word = _word_lm_table(word_lm, "beam_tlm")
            t.kind, t.word_lm = BEAM_TLM_WORD, ctypes.pointer(self._word)
            self._keep = (word_lm, ws)
        need = beam_tlm_ws_bytes(search.B, search.K)
        if not (ws.is_cuda and ws.is_contiguous() and ws.element_size() == 4 and ws.numel() * 4 >= need):
            raise RuntimeError("beam_tlm: an extra workspace of %d bytes on the GPU" % need)
        t.weight, t.bonus, t.lexicon_only = float(weight), float(bonus), 1 if lexicon_only else 0
        t.ws, t.ws_bytes = ptr(ws), ws.numel() * 4
        self.struct = t

    def _run(self, rc, what):
        if rc == ASR_E_SHAPE:
            raise UnsupportedShape("%s: refused the sizes or the LM's tables" % what)
        check(rc, what)

    def init(self):
        self._run(load().asr_beam_tlm_init_f32(ctypes.byref(self.search.struct), ctypes.byref(self.struct), stream()),
                  "asr_beam_tlm_init_f32")

    def select(self, logits, t, lm_logits=None, lm_weight=0.0, ctc=None, ctc_weight=0.0):
        """The select of step t with the LM's term: lm_logits [B*K, V] (the judge, shallow fusion) and ctc (CtcPrefixState
        after its score()) with ctc_weight as BeamSearch.select_lm / select_ctc take them."""
        self._run(load().asr_beam_select_tlm_f32(self.search._step(logits, lm_logits, ctc), ctypes.byref(self.struct),
                                                 ptr(lm_logits), float(lm_weight), ptr(ctc.psi) if ctc is not None else None,
                                                 ptr(ctc.psi_prev) if ctc is not None else None,
                                                 float(ctc_weight) if ctc is not None else 0.0, int(t), stream()),
                  "asr_beam_select_tlm_f32")

    def backtrack(self, length_penalty=0.0):
        """-> BeamSearch.backtrack's tokens, scores (the rank / len**length_penalty), lengths, and in the same order att_score
        fp32 [B, K] (base), lm_score fp32 [B, K], n int32 [B, K] (len, or n_words with a word LM; -1 without a hypothesis)."""
        s = self.search
        tokens, scores, lengths = s._hyps()
        att, lm, n = torch.empty_like(scores), torch.empty_like(scores), torch.empty_like(lengths)
        self._run(load().asr_beam_backtrack_tlm(ctypes.byref(s.struct), ctypes.byref(self.struct), float(length_penalty),
                                                ptr(tokens), ptr(scores), ptr(lengths), ptr(att), ptr(lm), ptr(n), stream()),
                  "asr_beam_backtrack_tlm")
        return tokens, scores, lengths, att, lm, n


class CtcPrefixState:
    """The CTC prefix scorer's state beside a BeamSearch (asr_ctc_prefix_t, csrc/ctc_prefix.hip): for the
    R = B*K beam rows state [2, R, Tp, 2] ((r_n, r_b) per frame, two slots), last [2, R] (the prefix's last token, -1 while
    it is empty), psi [R, V], psi_prev [R], and lse [B, Tp] - nothing that grows with the number of steps.
    logits [B, Tp, V] fp32 RAW CTC logits (a view with unit column stride and row stride >= V is taken as it is),
    frame_lens int32 [B] on the device; lens_host: the host's copy of them where it has one (checked: 1 .. Tp).
    The constructor runs the init kernel (slot 0 = the empty prefix); per step score() before the select, advance(t)
    after it - `cur` is the slot that holds the live prefixes."""

    def __init__(self, search, logits, frame_lens, blank=0, lens_host=None):
        B, Tp, V = logits.shape
        if (B, V) != (search.B, search.V):
            raise ValueError("CTC logits %s do not fit a search over %d utterances and %d tokens"
                             % (tuple(logits.shape), search.B, search.V))
        if frame_lens.dtype != torch.int32 or tuple(frame_lens.shape) != (B,):
            raise ValueError("frame_lens must be int32 [%d] on the device" % B)
        if not (logits.stride(2) == 1 and logits.stride(1) >= V and logits.stride(0) == Tp * logits.stride(1)):
            logits = logits.contiguous()
        dev = logits.device
        R = B * search.K
        f32 = dict(dtype=torch.float32, device=dev)
        self.search, self.logits, self.frame_lens, self.cur = search, _dev(logits, "ctc logits"), frame_lens, 0
        self.lse = torch.empty(B, Tp, **f32)
        self.state = torch.empty(2, R, Tp, 2, **f32)
        self.last = torch.empty(2, R, dtype=torch.int32, device=dev)
        self.psi = torch.full((R, V), float("-inf"), **f32)
        self.psi_prev = torch.empty(R, **f32)
        st = CtcPrefix(B=B, K=search.K, V=V, Tp=Tp, blank=blank, eos=search.eos, logits=ptr(self.logits),
                       ld=self.logits.stride(1), frame_lens=ptr(frame_lens), lse=ptr(self.lse), psi=ptr(self.psi),
                       psi_prev=ptr(self.psi_prev))
        for i in range(2):
            st.state[i], st.last[i] = self.state[i].data_ptr(), self.last[i].data_ptr()
        self.struct = st
        host = None
        if lens_host is not None:
            host = (ctypes.c_int32 * B)(*[int(n) for n in lens_host])
        rc = load().asr_ctc_prefix_init_f32(ctypes.byref(st), host, stream())
        if rc == ASR_E_SHAPE:
            raise UnsupportedShape("ctc prefix scorer: K %d, V %d, blank %d, eos %d, frames %s of %d (V >= 3, blank != eos, "
                                   "1 .. T' frames)" % (search.K, V, blank, search.eos, lens_host, Tp))
        check(rc, "asr_ctc_prefix_init_f32")

    def score(self):
        """psi [R, V] of the live rows' candidates from slot `cur` (rows that are dead or done keep what they hold)."""
        check(load().asr_ctc_prefix_score_f32(ctypes.byref(self.struct), ctypes.byref(self.search.struct), self.cur, stream()),
              "asr_ctc_prefix_score_f32")

    def advance(self, t):
        """After the select of step t: every live row's extended prefix, from its predecessor in slot `cur` into the other
        slot, which becomes `cur`."""
        check(load().asr_ctc_prefix_advance_f32(ctypes.byref(self.struct), ctypes.byref(self.search.struct), int(t), self.cur,
                                                1 - self.cur, stream()), "asr_ctc_prefix_advance_f32")
        self.cur = 1 - self.cur


ED_MAX_COLS = 4096         # ASR_ED_MAX_COLS


class UnsupportedShape(RuntimeError):
    """A launcher answered ASR_E_SHAPE: its kernel does not cover these sizes (the caller may have another route)."""


def _ints(t, name, dtypes, dim):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU: the HIP path has no CPU fallback" % name)
    if t.dtype not in dtypes:
        raise RuntimeError("%s must be %s, got %s" % (name, " or ".join(str(d) for d in dtypes), t.dtype))
    if t.dim() != dim or (t.shape[-1] > 1 and t.stride(-1) != 1):
        raise RuntimeError("%s must be %d-D with unit stride in its last dimension" % (name, dim))
    return c_p(t.data_ptr())


def _edit_distance(entry, space, hyp, ref, ref_len, hyp_len, ref_index, eos, skip, totals, out):
    """The argument checks and the launch that asr_edit_distance_i32 (space None) and asr_word_edit_distance_i32 share."""
    N = hyp.shape[0]
    hp = _ints(hyp, "hyp", (torch.int32, torch.int64), 2)
    rp, rlp = _ints(ref, "ref", (torch.int32,), 2), _ints(ref_len, "ref_len", (torch.int32,), 1)
    hlp, rip = _ints(hyp_len, "hyp_len", (torch.int32,), 1), _ints(ref_index, "ref_index", (torch.int32,), 1)
    sp, tp = _ints(skip, "skip", (torch.uint8,), 1), _ints(totals, "totals", (torch.int64,), 1)
    if ref_len.shape[0] != ref.shape[0] or (ref_index is None and ref.shape[0] < N):
        raise RuntimeError("ref has %d rows, ref_len %d, for %d pairs" % (ref.shape[0], ref_len.shape[0], N))
    for t, n, name in ((hyp_len, N, "hyp_len"), (ref_index, N, "ref_index"), (totals, 2, "totals")):
        if t is not None and t.shape[0] != n:
            raise RuntimeError("%s must have %d entries, got %d" % (name, n, t.shape[0]))
    if out is None:
        out = torch.empty(3, N, dtype=torch.int32, device=hyp.device)
    op = _ints(out, "out", (torch.int32,), 2)
    if tuple(out.shape) != (3, N) or not out.is_contiguous():
        raise RuntimeError("out must be a contiguous int32 [3, %d]" % N)
    rc = getattr(load(), entry)(
        N, hp, hyp.element_size(), hyp.stride(0) if N > 1 else max(hyp.shape[1], 1), hyp.shape[1], hlp, rp,
        ref.stride(0) if ref.shape[0] > 1 else max(ref.shape[1], 1), rlp, rip, int(eos), sp,
        0 if skip is None else skip.shape[0], *(() if space is None else (int(space),)),
        op, c_p(out[1].data_ptr()), c_p(out[2].data_ptr()), tp, stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("%s: more than %d columns (hyp %d, ref %d)" % (entry, ED_MAX_COLS, hyp.shape[1], ref.shape[1]))
    check(rc, entry)
    return out[0], out[1], out[2]


def edit_distance(hyp, ref, ref_len, *, hyp_len=None, ref_index=None, eos=-1, skip=None, totals=None, out=None):
    """asr_edit_distance_i32 (csrc/edit_distance.hip): the Levenshtein distance of every hypothesis row to its reference row
    on token ids, one launch.  hyp [N, cols] int32 or int64 (row p runs to hyp_len[p], int32 [N]; None: to cols; cut before
    its first `eos` unless eos < 0); ref [R, cols] int32 with ref_len int32 [R]; pair p scores against reference row p, or
    ref_index[p] (int32 [N]: K hypotheses per reference); skip: uint8 [V], tokens with a non-zero entry are dropped from
    both sides (utils.cer_token_table); totals: int64 [2], += (sum of distances, sum of reference lengths).
    -> (dist, hyp_n, ref_n), int32 [N] device tensors: distance and the two filtered lengths - rows of `out` (int32 [3, N])
    when it is given.  Raises UnsupportedShape beyond ED_MAX_COLS columns: there is no other device path."""
    return _edit_distance("asr_edit_distance_i32", None, hyp, ref, ref_len, hyp_len, ref_index, eos, skip, totals, out)


def word_edit_distance(hyp, ref, ref_len, space, *, hyp_len=None, ref_index=None, eos=-1, skip=None, totals=None, out=None):
    """asr_word_edit_distance_i32 (csrc/edit_distance.hip): edit_distance on WORDS, one launch.  The arguments
    are edit_distance's; `space` is the id that separates words: after the cut and the filter a word is a maximal run of
    tokens other than `space` (str.split() of the rendered text), and two words are equal iff their tokens are.
    -> (dist, hyp_n, ref_n): the word-level distance and the two word counts; totals += (sum of distances, sum of reference
    word counts).  A negative `space` is an error of the call; UnsupportedShape beyond ED_MAX_COLS columns."""
    return _edit_distance("asr_word_edit_distance_i32", space, hyp, ref, ref_len, hyp_len, ref_index, eos, skip, totals, out)


def lm_step(R, H, In, xin, wcat, bcat, c_prev, c_out, h_out, h_out2=None):
    """asr_lm_step_f32: one LSTM layer step for R rows.  xin [R, >= In+H] rows [x | h_prev]; wcat [4H, In+H], bcat [4H]
    gate-interleaved; c_prev, c_out [R, H]; h_out (and h_out2) 2-D views with unit column stride that take h_new.
    Raises for widths the kernel does not serve (code -2): there is no other path."""
    check(load().asr_lm_step_f32(int(R), int(H), int(In), ptr(xin), xin.stride(0), ptr(wcat), ptr(bcat), ptr(c_prev),
                                 ptr(c_out), ptr(h_out), h_out.stride(0), ptr(h_out2),
                                 0 if h_out2 is None else h_out2.stride(0), stream()), "asr_lm_step_f32")


class LmStepState:
    """The judge LM's state for R rows of a beam search, two step slots per layer: xin[l] [2, R, In_l + H]
    input rows [x | h] and cell[l] [2, R, H]; slot 0 is what a step reads, slot 1 what it writes (the reorder gathers slot
    1 back into slot 0), so memory does not depend on the number of steps.  Weights are packed once here:
    wcat[l] [4H, In_l + H] = [W_ih | W_hh] and bcat[l] = b_ih + b_hh, rows gate-interleaved (unit * 4 + gate).
    `layers`: [(w_ih, w_hh, b_ih, b_hh)] per layer (LM.LSTM.direction_params), `emb` the LM's embedding table."""

    def __init__(self, R, emb, layers, device=None):
        device = emb.device if device is None else device
        n = len(layers)
        if not 1 <= n <= LM_MAX_LAYERS:
            raise ValueError("%d LM layers outside 1..%d" % (n, LM_MAX_LAYERS))
        if not 1 <= R <= LM_MAX_ROWS:
            raise ValueError("%d beam rows outside 1..%d: the LM step kernel does not serve them" % (R, LM_MAX_ROWS))
        f32 = dict(device=device, dtype=torch.float32)
        self.R, self.n, self.H = R, n, layers[0][1].shape[1]
        self.emb = emb.detach().contiguous()
        self.in_dim, self.xin, self.cell, self.wcat, self.bcat = [], [], [], [], []
        with torch.no_grad():
            for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(layers):
                H, In = self.H, w_ih.shape[1]
                want = self.emb.shape[1] if l == 0 else H
                if tuple(w_hh.shape) != (4 * H, H) or w_ih.shape[0] != 4 * H or In != want:
                    raise ValueError("LM layer %d: weights %s / %s do not stack on input width %d, hidden width %d"
                                     % (l, tuple(w_ih.shape), tuple(w_hh.shape), want, H))
                self.in_dim.append(In)
                self.xin.append(torch.zeros(2, R, In + H, **f32))
                self.cell.append(torch.zeros(2, R, H, **f32))
                w = torch.cat([w_ih.detach(), w_hh.detach()], dim=1).view(4, H, In + H)
                self.wcat.append(w.transpose(0, 1).reshape(4 * H, In + H).contiguous())
                self.bcat.append((b_ih.detach() + b_hh.detach()).view(4, H).t().contiguous().view(-1))
        self._reorder = None

    def prime(self, token):
        """Step 0's input: zero state (as allocated), `token` (<BOS>) in every row."""
        self.xin[0][0, :, :self.in_dim[0]] = self.emb[token]

    def step(self):
        """All layers, slot 0 -> slot 1: one launch per layer.  Layer l also writes its h into layer l+1's x part."""
        for l in range(self.n):
            In = self.in_dim[l]
            nxt = self.xin[l + 1][0][:, :self.H] if l + 1 < self.n else None
            lm_step(self.R, self.H, In, self.xin[l][0], self.wcat[l], self.bcat[l], self.cell[l][0], self.cell[l][1],
                    self.xin[l][1][:, In:], nxt)

    def top(self):
        """[R, H] view (row stride In + H) of the last layer's new h: the operand of the LM's output layer."""
        return self.xin[-1][1][:, self.in_dim[-1]:]

    def reorder_struct(self):
        if self._reorder is None:
            st = BeamLmState(n_layers=self.n, H=self.H, emb=ptr(self.emb))
            for l in range(self.n):
                st.in_dim[l] = self.in_dim[l]
                st.x_src[l], st.x_dst[l] = self.xin[l][1].data_ptr(), self.xin[l][0].data_ptr()
                st.c_src[l], st.c_dst[l] = self.cell[l][1].data_ptr(), self.cell[l][0].data_ptr()
            self._reorder = st
        return self._reorder


FEED_PREDICTED, FEED_SMOOTH, FEED_TEACHER, FEED_NONE = 0, 1, 2, 3


def _lptr(t):
    return None if t is None else c_p(t.data_ptr())


def dec_feedback_fwd(x_top, w_out, b_out, emb_w, logits, pred, mode, scaling=1.0, tok=None, fed=None, probs=None,
                     x_emb_next=None, xd_emb_next=None, mask=None):
    """One decoder step's output side (model.py:329-351): logits = x_top w_out^T + b, pred = argmax, and the next
    step's embedding input (teacher token / predicted token / softmax(scaling*logits) @ E), with its dropped-out copy.
    x_top [B, D+O] and the embedding slots are row-strided views of the step input buffer; pred/fed/tok are int64."""
    _dev(x_top, "x_top")
    B, DO = x_top.shape
    V, E = emb_w.shape
    ldx = x_top.stride(0)
    assert x_top.stride(1) == 1 and w_out.is_contiguous() and emb_w.is_contiguous() and logits.is_contiguous()
    tok_stride = 0
    if tok is not None:
        assert tok.dim() == 1 and tok.dtype == torch.long and tok.shape[0] == B
        tok_stride = tok.stride(0)
    for t in (pred, fed):
        assert t is None or (t.dtype == torch.long and t.is_contiguous() and t.numel() == B)
    ldm = 0
    if x_emb_next is not None:
        assert x_emb_next.stride(0) == ldx and x_emb_next.stride(1) == 1 and x_emb_next.shape == (B, E)
    if xd_emb_next is not None:
        assert xd_emb_next.stride(0) == ldx and xd_emb_next.stride(1) == 1 and mask.stride(1) == 1
        ldm = mask.stride(0)
    check(load().asr_dec_feedback_fwd(B, V, E, DO, ptr(x_top), ldx, ptr(w_out), ptr(b_out), ptr(emb_w), ptr(logits),
                                      _lptr(pred), int(mode), float(scaling), _lptr(tok), tok_stride, _lptr(fed),
                                      ptr(probs), ptr(x_emb_next), ptr(xd_emb_next), ptr(mask), ldm, stream()),
          "asr_dec_feedback_fwd")


def dec_feedback_bwd(demb, gtop, probs, emb_w, w_out, scaling, dlog):
    """Backward of the smooth embedding feedback: demb [B,E] (grad of step s's embedding input) -> dlog [B,V] (+=, grad
    of logits_{s-1}) -> gtop [B,D+O] (+=, grad of [z_{s-1}, c_{s-1}])."""
    _dev(demb, "demb")
    B, E = demb.shape
    V, DO = w_out.shape
    ldg = demb.stride(0)
    assert demb.stride(1) == 1 and gtop.stride(1) == 1 and gtop.stride(0) == ldg and gtop.shape == (B, DO)
    assert probs.is_contiguous() and dlog.is_contiguous() and w_out.is_contiguous() and emb_w.is_contiguous()
    check(load().asr_dec_feedback_bwd(B, V, E, DO, ptr(demb), ptr(gtop), ldg, ptr(probs), ptr(emb_w), ptr(w_out),
                                      float(scaling), ptr(dlog), stream()), "asr_dec_feedback_bwd")


CTC_MAX_LABELS = 1023     # ASR_CTC_MAX_LABELS


def ctc_ws_bytes(B, T, V, max_label_len):
    """asr_ctc_ws_bytes on plain integers (no tensors, no GPU) -> the workspace bytes of a CTC call; UnsupportedShape for
    sizes the kernels refuse (more than CTC_MAX_LABELS labels, V < 2)."""
    need = c_i64(0)
    rc = load().asr_ctc_ws_bytes(int(B), int(T), int(V), int(max_label_len), ctypes.byref(need))
    if rc == -2:
        raise UnsupportedShape("ctc_loss: B %d, T %d, V %d, %d labels (at most %d labels, V >= 2)"
                               % (B, T, V, max_label_len, CTC_MAX_LABELS))
    check(rc, "asr_ctc_ws_bytes")
    return need.value


def _ctc_args(logits, ld, frame_lens, labels, label_offsets, max_label_len, zero_infinity):
    B, T, V = logits.shape
    if labels.dtype != torch.long or not labels.is_cuda:
        raise RuntimeError("ctc_loss: labels must be one packed int64 tensor on the GPU")
    return (B, T, V, ptr(logits), int(ld), ptr(frame_lens), c_p(labels.data_ptr()), ptr(label_offsets), int(max_label_len),
            int(bool(zero_infinity)))


def ctc_loss_fwd(logits, ld, frame_lens, labels, label_offsets, max_label_len, zero_infinity, nll, ws):
    """asr_ctc_loss_fwd: logits [B, T, V] fp32 with row stride ld (a view of a wider buffer is fine), frame_lens int32 [B],
    labels packed int64, label_offsets int32 [B + 1], all on the device; nll [B] and the workspace ws (a float32 tensor of at
    least ctc_ws_bytes bytes) are the caller's.  The workspace goes to ctc_loss_bwd unchanged."""
    args = _ctc_args(logits, ld, frame_lens, labels, label_offsets, max_label_len, zero_infinity)
    check(load().asr_ctc_loss_fwd(*args, ptr(nll), ptr(ws), ws.numel() * 4, stream()), "asr_ctc_loss_fwd")
    LAUNCHES["ctc_loss"] += 1
    return nll


def ctc_loss_bwd(logits, ld, frame_lens, labels, label_offsets, max_label_len, zero_infinity, grad_nll, ws, dlogits, lddz):
    """asr_ctc_loss_bwd behind a ctc_loss_fwd with the same arguments and workspace: dlogits [B, T, >= V] with row stride lddz
    gets grad_nll[b] d nll_b / d logits, exact zeros behind each utterance."""
    args = _ctc_args(logits, ld, frame_lens, labels, label_offsets, max_label_len, zero_infinity)
    check(load().asr_ctc_loss_bwd(*args, ptr(grad_nll), ptr(ws), ws.numel() * 4, ptr(dlogits), int(lddz), stream()),
          "asr_ctc_loss_bwd")
    LAUNCHES["ctc_loss_bwd"] += 1
    return dlogits


CTC_STAR_MAX_LABELS = 681     # ASR_CTC_STAR_MAX_LABELS: 3 L + 2 states within the CTC chains' 2 * 1023 + 1


def ctc_star_ws_bytes(B, T, V, max_label_len):
    """asr_ctc_star_ws_bytes on plain integers (no tensors, no GPU) -> the workspace bytes of a star CTC call; UnsupportedShape
    for sizes the kernels refuse (more than CTC_STAR_MAX_LABELS labels, V < 2)."""
    need = c_i64(0)
    rc = load().asr_ctc_star_ws_bytes(int(B), int(T), int(V), int(max_label_len), ctypes.byref(need))
    if rc == -2:
        raise UnsupportedShape("ctc_star_loss: B %d, T %d, V %d, %d labels (at most %d labels, V >= 2)"
                               % (B, T, V, max_label_len, CTC_STAR_MAX_LABELS))
    check(rc, "asr_ctc_star_ws_bytes")
    return need.value


def _ctc_star_args(logits, ld, frame_lens, labels, label_offsets, max_label_len, penalty, zero_infinity):
    B, T, V = logits.shape
    if labels.dtype != torch.long or not labels.is_cuda:
        raise RuntimeError("ctc_star_loss: labels must be one packed int64 tensor on the GPU")
    if penalty.dtype != torch.float32 or not penalty.is_cuda or penalty.shape != (B,) or not penalty.is_contiguous():
        raise RuntimeError("ctc_star_loss: penalty must be a contiguous fp32 [B] tensor on the GPU")
    return (B, T, V, ptr(logits), int(ld), ptr(frame_lens), c_p(labels.data_ptr()), ptr(label_offsets), int(max_label_len),
            ptr(penalty), int(bool(zero_infinity)))


def _star_ws(ws, ws_bytes):
    """(pointer, bytes) of a workspace tensor of any dtype on the GPU - the library checks alignment and size itself"""
    if not ws.is_cuda:
        raise RuntimeError("ctc_star_loss: the workspace must live on the GPU")
    return c_p(ws.data_ptr()), ws.numel() * ws.element_size() if ws_bytes is None else int(ws_bytes)


def ctc_star_loss_fwd(logits, ld, frame_lens, labels, label_offsets, max_label_len, penalty, zero_infinity, nll, ws,
                      ws_bytes=None):
    """asr_ctc_star_loss_fwd: ctc_loss_fwd's arguments plus penalty, fp32 [B] on the device (<= 0 or -inf: the caller's to
    check).  nll [B] and the workspace ws (at least ctc_star_ws_bytes bytes, 4-byte aligned; ws_bytes: what the library is
    told it holds, the tensor's size by default) are the caller's.  The workspace goes to ctc_star_loss_bwd unchanged."""
    args = _ctc_star_args(logits, ld, frame_lens, labels, label_offsets, max_label_len, penalty, zero_infinity)
    check(load().asr_ctc_star_loss_fwd(*args, ptr(nll), *_star_ws(ws, ws_bytes), stream()), "asr_ctc_star_loss_fwd")
    LAUNCHES["ctc_star_loss"] += 1
    return nll


def ctc_star_loss_bwd(logits, ld, frame_lens, labels, label_offsets, max_label_len, penalty, zero_infinity, grad_nll, ws,
                      dlogits, lddz, ws_bytes=None):
    """asr_ctc_star_loss_bwd behind a ctc_star_loss_fwd with the same arguments and workspace: dlogits [B, T, >= V] with row
    stride lddz gets grad_nll[b] d nll_b / d logits, exact zeros behind each utterance."""
    args = _ctc_star_args(logits, ld, frame_lens, labels, label_offsets, max_label_len, penalty, zero_infinity)
    check(load().asr_ctc_star_loss_bwd(*args, ptr(grad_nll), *_star_ws(ws, ws_bytes), ptr(dlogits), int(lddz), stream()),
          "asr_ctc_star_loss_bwd")
    LAUNCHES["ctc_star_loss_bwd"] += 1
    return dlogits


GTC_MAX_NODES = 2047          # ASR_GTC_MAX_NODES: the CTC chains' 2 * 1023 + 1 states
GTC_MAX_ARCS = 65536          # ASR_GTC_MAX_ARCS, per graph

_GTC_DTYPES = dict(node_off=torch.int32, lab=torch.int32, start=torch.float32, fin=torch.float32, in_ptr=torch.int32,
                   in_src=torch.int32, in_w=torch.float32, out_ptr=torch.int32, out_dst=torch.int32, out_w=torch.float32,
                   order=torch.int32, head=torch.int32)


def gtc_ws_bytes(B, T, V, max_nodes):
    """asr_gtc_ws_bytes on plain integers (no tensors, no GPU) -> the workspace bytes of a graph CTC call; UnsupportedShape
    for sizes the kernels refuse (more than GTC_MAX_NODES nodes, V < 2)."""
    need = c_i64(0)
    rc = load().asr_gtc_ws_bytes(int(B), int(T), int(V), int(max_nodes), ctypes.byref(need))
    if rc == -2:
        raise UnsupportedShape("gtc_loss: B %d, T %d, V %d, %d nodes (at most %d nodes, V >= 2)"
                               % (B, T, V, max_nodes, GTC_MAX_NODES))
    check(rc, "asr_gtc_ws_bytes")
    return need.value


def _gtc_table(table, rows, graph_of=None):
    """The device form of a graph table (gtc.GraphTable after .to(device)) -> (asr_gtc_graphs_t, graph_of int32 [rows] on
    the device: the caller's, or the table's own); the tensors stay the table's.  A table built on the device
    (gtc.DeviceGraphTable) passes the same checks from host-known numbers alone: its NN and A are the capacities its arrays
    were sized by, not counts read back."""
    t = GtcGraphs()
    shapes = dict(node_off=table.G + 1, lab=table.NN, start=table.NN, fin=table.NN, in_ptr=table.NN + 1,
                  in_src=max(table.A, 1), in_w=max(table.A, 1), out_ptr=table.NN + 1, out_dst=max(table.A, 1),
                  out_w=max(table.A, 1), order=table.NN, head=table.G * table.V)
    for name, dtype in _GTC_DTYPES.items():
        a = getattr(table, name)
        if not (isinstance(a, torch.Tensor) and a.is_cuda):
            raise RuntimeError("gtc_loss: the graph tables are not on the device (Graph.to(device))")
        if a.dtype != dtype or not a.is_contiguous() or a.numel() != shapes[name]:
            raise RuntimeError("gtc_loss: the table's %s must be a contiguous %s tensor of %d elements" % (name, dtype, shapes[name]))
        setattr(t, name, ptr(a))
    t.V, t.G, t.max_nodes, t.max_arcs = table.V, table.G, table.max_nodes, table.max_arcs
    if graph_of is None:
        graph_of = table.rows(rows)
    if not (graph_of.is_cuda and graph_of.dtype == torch.int32 and graph_of.is_contiguous() and graph_of.numel() == rows):
        raise RuntimeError("gtc_loss: graph_of must be a contiguous int32 tensor of %d rows on the device" % rows)
    return t, graph_of


def gtc_loss_fwd(logits, ld, frame_lens, table, zero_infinity, nll, ws, ws_bytes=None, graph_of=None):
    """asr_gtc_loss_fwd (csrc/gtc.hip): ctc_loss_fwd's arguments with a graph table on the device
    (gtc.GraphTable after .to(device); its own graph_of, or the caller's int32 [B]) in place of the labels.  nll [B] and the
    workspace ws (at least gtc_ws_bytes bytes, 4-byte aligned; ws_bytes: what the library is told it holds, the tensor's
    size by default) are the caller's.  The workspace goes to gtc_loss_bwd unchanged.  UnsupportedShape for a graph above
    GTC_MAX_NODES nodes or GTC_MAX_ARCS arcs."""
    B, T, V = logits.shape
    t, graph_of = _gtc_table(table, B, graph_of)
    rc = load().asr_gtc_loss_fwd(B, T, V, ptr(logits), int(ld), ptr(frame_lens), ctypes.byref(t), ptr(graph_of),
                                 int(bool(zero_infinity)), ptr(nll), *_star_ws(ws, ws_bytes), stream())
    if rc == -2:
        raise UnsupportedShape("gtc_loss: B %d, T %d, V %d, graphs of up to %d nodes and %d arcs (at most %d and %d, V >= 2)"
                               % (B, T, V, table.max_nodes, table.max_arcs, GTC_MAX_NODES, GTC_MAX_ARCS))
    check(rc, "asr_gtc_loss_fwd")
    LAUNCHES["gtc_loss"] += 1
    return nll


def gtc_loss_bwd(logits, ld, frame_lens, table, zero_infinity, grad_nll, ws, dlogits, lddz, ws_bytes=None, graph_of=None):
    """asr_gtc_loss_bwd behind a gtc_loss_fwd with the same arguments and workspace: dlogits [B, T, >= V] with row stride
    lddz gets grad_nll[b] d nll_b / d logits, exact zeros behind each utterance and for a row without a path."""
    B, T, V = logits.shape
    t, graph_of = _gtc_table(table, B, graph_of)
    check(load().asr_gtc_loss_bwd(B, T, V, ptr(logits), int(ld), ptr(frame_lens), ctypes.byref(t), ptr(graph_of),
                                  int(bool(zero_infinity)), ptr(grad_nll), *_star_ws(ws, ws_bytes), ptr(dlogits), int(lddz),
                                  stream()), "asr_gtc_loss_bwd")
    LAUNCHES["gtc_loss_bwd"] += 1
    return dlogits


def gtc_nbest_bytes(B, K, L, V):
    """asr_nbest_gtc_bytes on plain integers (no tensors, no GPU) -> (cap_nodes, cap_arcs, workspace bytes) of an n-best graph
    build: the per-row capacities its table is sized by; UnsupportedShape for K outside 1 .. BEAM_KMAX, V outside 2 .. 2**20
    or a batch whose arrays would pass the int32 offsets."""
    cn, ca, need = ctypes.c_int32(0), ctypes.c_int32(0), c_i64(0)
    rc = load().asr_nbest_gtc_bytes(int(B), int(K), int(L), int(V), ctypes.byref(cn), ctypes.byref(ca), ctypes.byref(need))
    if rc == -2:
        raise UnsupportedShape("gtc_nbest_graphs: B %d, K %d, L %d, V %d (K in 1..%d, V in 2..2**20)" % (B, K, L, V, BEAM_KMAX))
    check(rc, "asr_nbest_gtc_bytes")
    return cn.value, ca.value, need.value


def gtc_nbest(hyp, hyp_len, score, temperature, table, log_weights, dropped, ws):
    """asr_nbest_gtc_f32 (csrc/gtc_nbest.hip): the n-best list of ctc_beam - hyp int32 [B, K, L], hyp_len int32
    [B, K], score fp32 [B, K] on the device - compiled into `table`, a gtc.DeviceGraphTable whose capacity-sized arrays (and
    graph_of) the call writes; log_weights fp64 [B, K], dropped int32 [B] and the workspace (gtc_nbest_bytes) are the
    caller's.  Two launches, no host synchronisation."""
    B, K, L = hyp.shape
    for name, a, dtype, n in (("hyp", hyp, torch.int32, B * K * L), ("hyp_len", hyp_len, torch.int32, B * K),
                              ("score", score, torch.float32, B * K), ("log_weights", log_weights, torch.float64, B * K),
                              ("dropped", dropped, torch.int32, B)):
        if not (a.is_cuda and a.dtype == dtype and a.is_contiguous() and a.numel() == n):
            raise RuntimeError("gtc_nbest_graphs: %s must be a contiguous %s tensor of %d elements on the device" % (name, dtype, n))
    t, graph_of = _gtc_table(table, B)
    rc = load().asr_nbest_gtc_f32(B, K, L, table.V, ptr(hyp), ptr(hyp_len), ptr(score), float(temperature), ctypes.byref(t),
                                  ptr(graph_of), c_p(log_weights.data_ptr()), ptr(dropped), *_star_ws(ws, None), stream())
    if rc == -2:
        raise UnsupportedShape("gtc_nbest_graphs: B %d, K %d, L %d, V %d (K in 1..%d, V in 2..2**20)" % (B, K, L, table.V, BEAM_KMAX))
    check(rc, "asr_nbest_gtc_f32")
    LAUNCHES["gtc_nbest"] += 1
    return table


RNNT_MAX_LABELS = 1023       # ASR_RNNT_MAX_LABELS


def rnnt_ws_bytes(B, T, U, J, V):
    """asr_rnnt_ws_bytes on plain integers (no tensors, no GPU) -> the workspace bytes of an rnnt_loss call over B utterances
    of at most T frames and U labels, joint width J, vocabulary V; UnsupportedShape for sizes the kernels refuse (V < 2, J not
    a multiple of 4, more than RNNT_MAX_LABELS labels, a node matrix B T (U + 1) max(J, V) the launches cannot cover)."""
    need = c_i64(0)
    rc = load().asr_rnnt_ws_bytes(int(B), int(T), int(U), int(J), int(V), ctypes.byref(need))
    if rc == -2:
        raise UnsupportedShape("rnnt: B %d, T %d, U %d, J %d, V %d (V >= 2, J a multiple of 4, at most %d labels, "
                               "B T (U + 1) max(J, V) <= 2^40)" % (B, T, U, J, V, RNNT_MAX_LABELS))
    check(rc, "asr_rnnt_ws_bytes")
    return int(need.value)


def _rnnt_lens(frame_lens, label_offsets, B):
    if frame_lens.dtype != torch.int32 or label_offsets.dtype != torch.int32 or frame_lens.numel() != B or \
            label_offsets.numel() != B + 1:
        raise RuntimeError("rnnt: frame_lens int32 [B] and label_offsets int32 [B + 1] on the GPU")


def rnnt_joint_fwd(pe, pp, frame_lens, label_offsets, z):
    """asr_rnnt_joint_fwd_f32: z [B, T, U + 1, J] = tanh(pe [B, T, J] + pp [B, U + 1, J]) on the lattice of every utterance,
    exact zeros on padding.  All contiguous; z is the caller's.  UnsupportedShape before anything is written."""
    B, T, J = pe.shape
    U = pp.shape[1] - 1
    if tuple(pp.shape) != (B, U + 1, J) or tuple(z.shape) != (B, T, U + 1, J) or not (pe.is_contiguous() and pp.is_contiguous()
                                                                                      and z.is_contiguous()):
        raise RuntimeError("rnnt_joint_fwd: pe [B, T, J], pp [B, U + 1, J], z [B, T, U + 1, J], contiguous")
    _rnnt_lens(frame_lens, label_offsets, B)
    rnnt_ws_bytes(B, T, U, J, 2)
    check(load().asr_rnnt_joint_fwd_f32(B, T, U, J, ptr(pe), ptr(pp), ptr(frame_lens), ptr(label_offsets), ptr(z), stream()),
          "asr_rnnt_joint_fwd_f32")
    LAUNCHES["rnnt_joint"] += 1
    return z


def rnnt_joint_bwd(dz, z, frame_lens, label_offsets, dpe, dpp):
    """asr_rnnt_joint_bwd_f32: dz (1 - z^2) summed in a fixed order into dpe [B, T, J] and dpp [B, U + 1, J] (the caller's)."""
    B, T, U1, J = z.shape
    if tuple(dz.shape) != (B, T, U1, J) or tuple(dpe.shape) != (B, T, J) or tuple(dpp.shape) != (B, U1, J) or \
            not (dz.is_contiguous() and z.is_contiguous() and dpe.is_contiguous() and dpp.is_contiguous()):
        raise RuntimeError("rnnt_joint_bwd: dz, z [B, T, U + 1, J], dpe [B, T, J], dpp [B, U + 1, J], contiguous")
    _rnnt_lens(frame_lens, label_offsets, B)
    rnnt_ws_bytes(B, T, U1 - 1, J, 2)
    check(load().asr_rnnt_joint_bwd_f32(B, T, U1 - 1, J, ptr(dz), ptr(z), ptr(frame_lens), ptr(label_offsets), ptr(dpe), ptr(dpp),
                                        stream()), "asr_rnnt_joint_bwd_f32")
    LAUNCHES["rnnt_joint_bwd"] += 1
    return dpe, dpp


def _rnnt_loss_args(logits, ld, frame_lens, labels, label_offsets):
    B, T, U1, V = logits.shape
    if labels.dtype != torch.int64 or not labels.is_cuda:
        raise RuntimeError("rnnt_loss: labels must be one packed int64 tensor on the GPU")
    _rnnt_lens(frame_lens, label_offsets, B)
    return (B, T, U1 - 1, V, ptr(logits), int(ld), ptr(frame_lens), c_p(labels.data_ptr()), ptr(label_offsets))


def rnnt_loss_fwd(logits, ld, frame_lens, labels, label_offsets, nll, ws):
    """asr_rnnt_loss_fwd_f32: raw logits [B, T, U + 1, V] fp32 with row stride ld (a view of a wider buffer is fine), frame_lens
    int32 [B], labels int64 packed, label_offsets int32 [B + 1] - all on the device; nll [B] and ws (a float32 tensor of at
    least rnnt_ws_bytes bytes) are the caller's.  The workspace goes to rnnt_loss_bwd unchanged."""
    args = _rnnt_loss_args(logits, ld, frame_lens, labels, label_offsets)
    rnnt_ws_bytes(args[0], args[1], args[2], 4, args[3])
    check(load().asr_rnnt_loss_fwd_f32(*args, ptr(nll), ptr(ws), ws.numel() * 4, stream()), "asr_rnnt_loss_fwd_f32")
    LAUNCHES["rnnt_loss"] += 1
    return nll


def rnnt_loss_bwd(logits, ld, frame_lens, labels, label_offsets, grad_nll, ws, dlogits, lddz):
    """asr_rnnt_loss_bwd_f32 behind an rnnt_loss_fwd with the same arguments and workspace: dlogits [B, T, U + 1, >= V] with
    row stride lddz, zeros on padding."""
    args = _rnnt_loss_args(logits, ld, frame_lens, labels, label_offsets)
    check(load().asr_rnnt_loss_bwd_f32(*args, ptr(grad_nll), ptr(ws), ws.numel() * 4, ptr(dlogits), int(lddz), stream()),
          "asr_rnnt_loss_bwd_f32")
    LAUNCHES["rnnt_loss_bwd"] += 1
    return dlogits


def rnnt_greedy_step(pe, pp, w_out, b_out, frame_lens, t_cur, n_out, n_frame, out, last, score, advance, max_symbols):
    """asr_rnnt_greedy_step_f32: one iteration of transducer greedy decoding for all rows (include/asr_hip.h).  pe [B, T, J],
    pp [B, J], w_out [V, J], b_out [V] or None; the state - t_cur, n_out, n_frame, last, advance int32 [B], out int32 [B, L],
    score fp32 [B] - lives on the device.  The argmax takes the lower index on ties."""
    B, T, J = pe.shape
    V, L = w_out.shape[0], out.shape[1]
    state = (t_cur, n_out, n_frame, last, advance)
    if tuple(pp.shape) != (B, J) or w_out.shape[1] != J or tuple(out.shape) != (B, L) or score.numel() != B or \
            any(s.dtype != torch.int32 or s.numel() != B for s in state) or out.dtype != torch.int32 or \
            not all(x.is_contiguous() for x in (pe, pp, w_out, out)):
        raise RuntimeError("rnnt_greedy_step: pe [B, T, J], pp [B, J], w_out [V, J], int32 state [B], out int32 [B, L], contiguous")
    rc = load().asr_rnnt_greedy_step_f32(B, T, J, V, L, int(max_symbols), ptr(pe), ptr(pp), ptr(w_out), ptr(b_out),
                                         ptr(frame_lens), ptr(t_cur), ptr(n_out), ptr(n_frame), ptr(out), ptr(last), ptr(score),
                                         ptr(advance), stream())
    if rc == -2:
        raise UnsupportedShape("rnnt_greedy_step: J %d, V %d (V >= 2, J a multiple of 4, (J + V) floats within 64 KB)" % (J, V))
    check(rc, "asr_rnnt_greedy_step_f32")
    LAUNCHES["rnnt_greedy_step"] += 1


def rnnt_align_ws_bytes(B, T, U, V):
    """asr_transducer_align_ws_bytes on plain integers (no tensors, no GPU) -> the workspace bytes of an rnnt_align call over B
    utterances of at most T frames and U labels, vocabulary V; UnsupportedShape for sizes the kernels refuse (V < 2, more
    than RNNT_MAX_LABELS labels, a node matrix beyond rnnt_ws_bytes's bounds)."""
    need = c_i64(0)
    rc = load().asr_transducer_align_ws_bytes(int(B), int(T), int(U), int(V), ctypes.byref(need))
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("rnnt_align: B %d, T %d, U %d, V %d (V >= 2, at most %d labels, B T (U + 1) max(4, V) <= 2^40)"
                               % (B, T, U, V, RNNT_MAX_LABELS))
    check(rc, "asr_transducer_align_ws_bytes")
    return int(need.value)


def rnnt_align(logits, ld, frame_lens, labels, label_offsets, score, emit_frame, token_logp, frame_labels, blank_logp, ws):
    """asr_transducer_align_f32 (csrc/rnnt_align.hip): the best alignment of every utterance's labels on the
    transducer lattice.  The inputs are rnnt_loss_fwd's; the outputs score fp32 [B], emit_frame int32 and token_logp fp32
    (packed like labels), frame_labels int32 [B, T], blank_logp fp32 [B, T] and the workspace ws (a float32 tensor of at
    least rnnt_align_ws_bytes bytes) are the caller's.  Two launches."""
    args = _rnnt_loss_args(logits, ld, frame_lens, labels, label_offsets)
    B, T = args[0], args[1]
    if emit_frame.dtype != torch.int32 or frame_labels.dtype != torch.int32 or emit_frame.numel() != token_logp.numel() or \
            score.numel() != B or tuple(frame_labels.shape) != (B, T) or tuple(blank_logp.shape) != (B, T) or \
            not (frame_labels.is_contiguous() and blank_logp.is_contiguous()):
        raise RuntimeError("rnnt_align: score [B], emit_frame int32 / token_logp packed like labels, frame_labels int32 and "
                           "blank_logp [B, T], contiguous")
    rnnt_align_ws_bytes(B, T, args[2], args[3])
    check(load().asr_transducer_align_f32(*args, ptr(score), ptr(emit_frame), ptr(token_logp), ptr(frame_labels), ptr(blank_logp),
                                    ptr(ws), ws.numel() * 4, stream()), "asr_transducer_align_f32")
    LAUNCHES["rnnt_align"] += 1
    LAUNCHES["rnnt_align_launch"] += 2


RNNT_BEAM_LDS_BYTES = 56 * 1024      # ASR_RNNT_BEAM_LDS_BYTES: K (J + V) floats of the step kernel's LDS


def rnnt_beam_ws_bytes(B, T, J, V, K, L, E, P):
    """asr_transducer_beam_ws_bytes on plain integers (no tensors, no GPU) -> the workspace bytes of a transducer beam search;
    UnsupportedShape for sizes the kernels refuse."""
    need = c_i64(0)
    rc = load().asr_transducer_beam_ws_bytes(int(B), int(T), int(J), int(V), int(K), int(L), int(E), int(P), ctypes.byref(need))
    if rc == -2:
        raise UnsupportedShape("rnnt_beam: B %d, T %d, J %d, V %d, beam %d, L %d (beam 1 .. %d, V >= 2, J a multiple of 4, "
                               "beam (J + V) floats within %d bytes of LDS)" % (B, T, J, V, K, L, BEAM_KMAX, RNNT_BEAM_LDS_BYTES))
    check(rc, "asr_transducer_beam_ws_bytes")
    return need.value


class RnntBeam(object):
    """One transducer beam search (csrc/rnnt_beam.hip) over the caller's tensors: pe [B, T, J], w_out [V, J],
    b_out [V] or None, emb [V, E], frame_lens int32 [B]; the state h, c [B K, P], xh [B K, E + P], pp [B K, J] and the
    workspace ws (float32, at least rnnt_beam_ws_bytes bytes) are the caller's too, all contiguous fp32 on the device.  table:
    the n-gram LM on the device or None.  init(), then per iteration step(it) - between them the caller runs the gate
    product, cell() and the projection - and backtrace() behind the loop.  Every method is one launch."""

    COUNT = "rnnt_beam"                  # LAUNCHES[COUNT + "_launch"] counts every launch of a search

    def __init__(self, pe, w_out, b_out, emb, frame_lens, K, L, h, c, xh, pp, ws, table=None, alpha=0.0, beta=0.0,
                 eos_term=True):
        B, T, J = pe.shape
        V, E, P = w_out.shape[0], emb.shape[1], h.shape[1]
        K, L = int(K), int(L)
        floats = [pe, w_out, emb, h, c, xh, pp, ws] + ([b_out] if b_out is not None else [])
        if any(not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()) for t in floats) or \
                not (frame_lens.is_cuda and frame_lens.dtype == torch.int32 and frame_lens.numel() == B):
            raise RuntimeError("rnnt_beam: contiguous fp32 tensors and frame_lens int32 [B] on the GPU")
        need = rnnt_beam_ws_bytes(B, T, J, V, K, L, E, P)
        if tuple(w_out.shape) != (V, J) or emb.shape[0] != V or tuple(h.shape) != (B * K, P) or tuple(c.shape) != (B * K, P) or \
                tuple(xh.shape) != (B * K, E + P) or tuple(pp.shape) != (B * K, J) or ws.numel() * 4 < need:
            raise RuntimeError("rnnt_beam: w_out [V, J], emb [V, E], h / c [B K, P], xh [B K, E + P], pp [B K, J] and a "
                               "workspace of %d bytes" % need)
        a = RnntBeamArgs()
        a.B, a.T, a.J, a.V, a.K, a.L, a.E, a.P = B, T, J, V, K, L, E, P
        a.pe, a.pp, a.w_out, a.b_out, a.emb, a.frame_lens = ptr(pe), ptr(pp), ptr(w_out), ptr(b_out), ptr(emb), ptr(frame_lens)
        a.h, a.c, a.xh, a.ws, a.ws_bytes = ptr(h), ptr(c), ptr(xh), ptr(ws), ws.numel() * 4
        if table is not None:
            logp, nxt, S = _ngram_table(table, V, "rnnt_beam")
            a.lm_logp, a.lm_next, a.lm_states, a.lm_start = ptr(logp), ptr(nxt), S, int(table.start)
            a.lm_eos, a.lm_alpha, a.lm_beta = (int(table.eos) if eos_term else -1), float(alpha), float(beta)
        else:
            a.lm_logp, a.lm_next, a.lm_states, a.lm_start, a.lm_eos, a.lm_alpha, a.lm_beta = None, None, 0, 0, -1, 0.0, 0.0
        self.args, self.B, self.K, self.L, self.h, self.c = a, B, K, L, h, c
        self._keep = (pe, w_out, b_out, emb, frame_lens, h, c, xh, pp, ws, table)

    def _run(self, rc, what):
        if rc == ASR_E_SHAPE:
            raise UnsupportedShape("%s: refused the sizes or the n-gram table" % what)
        check(rc, what)
        LAUNCHES[self.COUNT + "_launch"] += 1

    def init(self, bos):
        self._run(load().asr_transducer_beam_init_f32(ctypes.byref(self.args), int(bos), stream()), "asr_transducer_beam_init_f32")

    def step(self, it):
        self._run(load().asr_transducer_beam_step_f32(ctypes.byref(self.args), int(it), stream()), "asr_transducer_beam_step_f32")
        LAUNCHES["rnnt_beam_step"] += 1

    def cell(self, gates):
        if tuple(gates.shape) != (self.h.shape[0], 4 * self.h.shape[1]) or not gates.is_contiguous():
            raise RuntimeError("rnnt_beam: gates must be contiguous [B K, 4 P]")
        self._run(load().asr_transducer_beam_cell_f32(ctypes.byref(self.args), ptr(gates), ptr(self.h), ptr(self.c), stream()),
                  "asr_transducer_beam_cell_f32")

    def product(self, x, w, out, bias=None):
        """out = x w^T (+ bias) on asr_gemm_f32, unsplit: the same bits in and outside deterministic mode.  One launch."""
        gemm(x, w, trans_b=True, bias=bias, out=out, split_k=1)
        LAUNCHES[self.COUNT + "_launch"] += 1

    def backtrace(self, hyp, hyp_len, score, rnnt_score=None, lm_score=None):
        B, K, L = self.B, self.K, self.L
        outs = [hyp_len, score] + [t for t in (rnnt_score, lm_score) if t is not None]
        if tuple(hyp.shape) != (B, K, L) or hyp.dtype != torch.int32 or not hyp.is_contiguous() or \
                any(t.numel() != B * K or not t.is_contiguous() for t in outs):
            raise RuntimeError("rnnt_beam: hyp int32 [B, K, L], hyp_len / score [B, K], contiguous")
        self._run(load().asr_transducer_beam_backtrace_f32(ctypes.byref(self.args), ptr(hyp), ptr(hyp_len), ptr(score),
                                                     ptr(rnnt_score), ptr(lm_score), stream()),
                  "asr_transducer_beam_backtrace_f32")


def rnnt_wbeam_ws_bytes(B, K):
    """asr_transducer_wbeam_ws_bytes on plain integers (no tensors, no GPU) -> the EXTRA workspace bytes of a transducer beam
    search with a word LM inside: 4 * 7 * round64(B K); UnsupportedShape for a beam outside 1 .. BEAM_KMAX."""
    need = c_i64(0)
    rc = load().asr_transducer_wbeam_ws_bytes(int(B), int(K), ctypes.byref(need))
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("rnnt_wbeam: B %d, beam %d (beam 1 .. %d)" % (B, K, BEAM_KMAX))
    check(rc, "asr_transducer_wbeam_ws_bytes")
    return need.value


class RnntWordBeam(RnntBeam):
    """RnntBeam with a lexicon and a word-level LM inside the search (the asr_transducer_wbeam_* entries): table
    is the word LM on the device (word_lm.WordTable after .to(device)), wws the extra workspace (float32 or int32, at least
    rnnt_wbeam_ws_bytes bytes); candidates rank by (tot + alpha lm) + beta n_words.  cell() and product() are RnntBeam's;
    init(), step() and backtrace() are one launch each, counted under LAUNCHES["rnnt_wbeam_launch"]."""

    COUNT = "rnnt_wbeam"

    def __init__(self, pe, w_out, b_out, emb, frame_lens, K, L, h, c, xh, pp, ws, table, wws, alpha=0.0, beta=0.0,
                 eos_term=True, lexicon_only=False):
        RnntBeam.__init__(self, pe, w_out, b_out, emb, frame_lens, K, L, h, c, xh, pp, ws)
        V = w_out.shape[0]
        if table.V != V:
            raise UnsupportedShape("rnnt_wbeam: the word LM spells in %d tokens, the head is over %d" % (table.V, V))
        self.lm = _word_lm_table(table, "rnnt_wbeam")
        need = rnnt_wbeam_ws_bytes(self.B, self.K)
        if not (wws.is_cuda and wws.is_contiguous() and wws.element_size() == 4 and wws.numel() * 4 >= need):
            raise RuntimeError("rnnt_wbeam: an extra workspace of %d bytes on the GPU" % need)
        self._wargs = (ctypes.byref(self.lm), float(alpha), float(beta), 1 if eos_term else 0, 1 if lexicon_only else 0,
                       ptr(wws), wws.numel() * 4)
        self._keep += (table, wws)

    def init(self, bos):
        self._run(load().asr_transducer_wbeam_init_f32(ctypes.byref(self.args), *self._wargs, int(bos), stream()),
                  "asr_transducer_wbeam_init_f32")

    def step(self, it):
        self._run(load().asr_transducer_wbeam_step_f32(ctypes.byref(self.args), *self._wargs, int(it), stream()),
                  "asr_transducer_wbeam_step_f32")
        LAUNCHES["rnnt_wbeam_step"] += 1

    def backtrace(self, hyp, hyp_len, score, rnnt_score, lm_score, n_words):
        B, K, L = self.B, self.K, self.L
        outs = [hyp_len, score, rnnt_score, lm_score, n_words]
        if tuple(hyp.shape) != (B, K, L) or hyp.dtype != torch.int32 or not hyp.is_contiguous() or \
                n_words.dtype != torch.int32 or any(t.numel() != B * K or not t.is_contiguous() for t in outs):
            raise RuntimeError("rnnt_wbeam: hyp int32 [B, K, L], hyp_len / score / rnnt_score / lm_score / n_words [B, K], "
                               "contiguous")
        self._run(load().asr_transducer_wbeam_backtrace_f32(ctypes.byref(self.args), *self._wargs, ptr(hyp), ptr(hyp_len),
                                                            ptr(score), ptr(rnnt_score), ptr(lm_score), ptr(n_words), stream()),
                  "asr_transducer_wbeam_backtrace_f32")


def _mwer_dims(logits, tokens, B):
    L, R, V = logits.shape
    if tokens.dtype != torch.long or not tokens.is_cuda or tuple(tokens.shape) != (L, R) or not tokens.is_contiguous():
        raise RuntimeError("mwer_loss: tokens must be a contiguous int64 [L, R] tensor on the GPU")
    if logits.stride(2) != 1 or logits.stride(0) != R * logits.stride(1):
        raise RuntimeError("mwer_loss: logits must be [L, R, V] with unit column stride and one row stride")
    if B <= 0 or R % B:
        raise RuntimeError("mwer_loss: %d rows are not K hypotheses for each of %d utterances" % (R, B))
    return int(B), R // int(B), L, V, int(logits.stride(1))


def mwer_fwd(logits, tokens, npos, err, B, scale, seq_logp, post, coef, risk, loss, ws):
    """asr_mwer_fwd_f32 (csrc/mwer.hip): logits [L, R, V] fp32 time-major (R = B K rows r = b K + k; a row stride wider than V
    is fine), tokens int64 [L, R], npos / err int32 [R]; outputs seq_logp / post / coef [R], risk [B], loss [1] and the
    workspace ws (fp32, at least L R elements) are the caller's.  Raises UnsupportedShape for K above BEAM_KMAX."""
    Bk, K, L, V, ld = _mwer_dims(logits, tokens, B)
    rc = load().asr_mwer_fwd_f32(Bk, K, L, V, ptr(logits), ld, c_p(tokens.data_ptr()), ptr(npos), ptr(err), float(scale),
                                 ptr(seq_logp), ptr(post), ptr(coef), ptr(risk), ptr(loss), ptr(ws), ws.numel() * 4, stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("asr_mwer_fwd_f32: B %d, K %d, L %d (K at most %d)" % (Bk, K, L, BEAM_KMAX))
    check(rc, "asr_mwer_fwd_f32")
    LAUNCHES["mwer"] += 2


def mwer_bwd(logits, tokens, npos, coef, B, grad_loss, grad_scale, dlogits):
    """asr_mwer_bwd_f32 behind a mwer_fwd on the same inputs: dlogits [L, R, V] contiguous gets grad_loss (one device scalar)
    grad_scale d(sum_b risk_b) / d logits, exact zeros behind each hypothesis and in unused rows."""
    Bk, K, L, V, ld = _mwer_dims(logits, tokens, B)
    rc = load().asr_mwer_bwd_f32(Bk, K, L, V, ptr(logits), ld, c_p(tokens.data_ptr()), ptr(npos), ptr(coef), ptr(grad_loss),
                                 float(grad_scale), ptr(dlogits), V, stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("asr_mwer_bwd_f32: B %d, K %d, L %d (K at most %d)" % (Bk, K, L, BEAM_KMAX))
    check(rc, "asr_mwer_bwd_f32")
    LAUNCHES["mwer"] += 1
    return dlogits


CTC_ALIGN_LDS_BYTES = 40960     # ASR_CTC_ALIGN_LDS_BYTES: an utterance's back-pointers stay in LDS up to this size


def ctc_align_ws_bytes(B, T, V, max_label_len):
    """asr_ctc_align_ws_bytes on plain integers (no tensors, no GPU) -> the workspace bytes of a ctc_align call;
    UnsupportedShape for sizes the kernels refuse (more than CTC_MAX_LABELS labels, V < 2)."""
    need = c_i64(0)
    rc = load().asr_ctc_align_ws_bytes(int(B), int(T), int(V), int(max_label_len), ctypes.byref(need))
    if rc == -2:
        raise UnsupportedShape("ctc_align: B %d, T %d, V %d, %d labels (at most %d labels, V >= 2)"
                               % (B, T, V, max_label_len, CTC_MAX_LABELS))
    check(rc, "asr_ctc_align_ws_bytes")
    return need.value


def _ctc_view(logits, what):
    """A [B, T, V] fp32 view with unit column stride and row stride ld >= V goes in as it is -> (logits, ld)."""
    B, T, V = _dev(logits, what).shape
    if not (logits.stride(2) == 1 and logits.stride(1) >= V and logits.stride(0) == T * logits.stride(1)):
        logits = logits.contiguous()
    return logits, logits.stride(1)


def ctc_align(logits, frame_lens, labels, label_offsets, max_label_len, path, score, first, last, token_logp, ws):
    """asr_ctc_align_f32 (csrc/ctc_align.hip): the best CTC alignment of every utterance's labels.  logits
    [B, T, V] fp32 raw (a view with row stride >= V is taken as it is), frame_lens int32 [B], labels packed int64,
    label_offsets int32 [B + 1], all on the device; the outputs path int32 [B, T], score fp32 [B], first / last int32 and
    token_logp fp32 (packed like labels) and the workspace ws (a float32 tensor of at least ctc_align_ws_bytes bytes) are the
    caller's.  Two launches."""
    logits, ld = _ctc_view(logits, "ctc logits")
    B, T, V = logits.shape
    if labels.dtype != torch.long or not labels.is_cuda:
        raise RuntimeError("ctc_align: labels must be one packed int64 tensor on the GPU")
    rc = load().asr_ctc_align_f32(B, T, V, ptr(logits), int(ld), ptr(frame_lens), c_p(labels.data_ptr()), ptr(label_offsets),
                                  int(max_label_len), ptr(path), ptr(score), ptr(first), ptr(last), ptr(token_logp), ptr(ws),
                                  ws.numel() * 4, stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("ctc_align: B %d, T %d, V %d, %d labels (at most %d labels, V >= 2)"
                               % (B, T, V, max_label_len, CTC_MAX_LABELS))
    check(rc, "asr_ctc_align_f32")
    LAUNCHES["ctc_align"] += 1


def ctc_greedy(logits, frame_lens, ids, n, frame_tok):
    """asr_ctc_greedy_f32: best-path CTC decoding of raw logits [B, T, V] (a view with row stride >= V is taken as it is) ->
    ids int32 [B, T] (the hypothesis, padded with -1), n int32 [B] (its length), frame_tok int32 [B, T] (the argmax of every
    frame, -1 behind the utterance), all the caller's.  One launch."""
    logits, ld = _ctc_view(logits, "ctc logits")
    B, T, V = logits.shape
    rc = load().asr_ctc_greedy_f32(B, T, V, ptr(logits), int(ld), ptr(frame_lens), ptr(ids), ptr(n), ptr(frame_tok), stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("ctc_greedy: V %d (V >= 2)" % V)
    check(rc, "asr_ctc_greedy_f32")
    LAUNCHES["ctc_greedy"] += 1


CTC_SEG_MAX_LABELS = 8191       # ASR_CTC_SEG_MAX_LABELS: the labels of one recording's transcript


def ctc_segment_ws_bytes(B, T, V, max_label_len):
    """asr_ctc_segment_ws_bytes on plain integers (no tensors, no GPU) -> the workspace bytes of a ctc_segment call;
    UnsupportedShape for sizes the kernel refuses (more than CTC_SEG_MAX_LABELS labels, V < 2)."""
    need = c_i64(0)
    rc = load().asr_ctc_segment_ws_bytes(int(B), int(T), int(V), int(max_label_len), ctypes.byref(need))
    if rc == -2:
        raise UnsupportedShape("ctc_segment: B %d, T %d, V %d, %d labels (at most %d labels, V >= 2)"
                               % (B, T, V, max_label_len, CTC_SEG_MAX_LABELS))
    check(rc, "asr_ctc_segment_ws_bytes")
    return need.value


def ctc_segment(logits, frame_lens, labels, label_offsets, max_label_len, free_ends, utt_offsets, rec_utts, window, path, score,
                first, last, token_logp, utt_begin, utt_end, utt_logp, utt_conf, ws):
    """asr_ctc_segment_f32 (csrc/ctc_segment.hip): the best CTC alignment of every recording's transcript, with
    free ends when free_ends is set, and the begin / end / log-probability / confidence of its utterances.  logits, frame_lens,
    labels, label_offsets, max_label_len and the outputs path .. token_logp are ctc_align's; utt_offsets int32 [N + 1] and
    rec_utts int32 [B + 1] on the device (the utterances' label ranges tile their recording's: the caller's duty); utt_begin /
    utt_end int32 [N], utt_logp / utt_conf fp32 [N] and the workspace ws (a float32 tensor of at least ctc_segment_ws_bytes
    bytes) are the caller's.  Two launches."""
    logits, ld = _ctc_view(logits, "ctc logits")
    B, T, V = logits.shape
    if labels.dtype != torch.long or not labels.is_cuda:
        raise RuntimeError("ctc_segment: labels must be one packed int64 tensor on the GPU")
    rc = load().asr_ctc_segment_f32(B, T, V, ptr(logits), int(ld), ptr(frame_lens), c_p(labels.data_ptr()), ptr(label_offsets),
                                    int(max_label_len), int(bool(free_ends)), int(utt_begin.numel()), ptr(utt_offsets),
                                    ptr(rec_utts), int(window), ptr(path), ptr(score), ptr(first), ptr(last), ptr(token_logp),
                                    ptr(utt_begin), ptr(utt_end), ptr(utt_logp), ptr(utt_conf), ptr(ws), ws.numel() * 4, stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("ctc_segment: B %d, T %d, V %d, %d labels (at most %d labels, V >= 2)"
                               % (B, T, V, max_label_len, CTC_SEG_MAX_LABELS))
    check(rc, "asr_ctc_segment_f32")
    LAUNCHES["ctc_segment"] += 1


CTC_BEAM_ONE_WAVE_KV = 1024      # ASR_CTC_BEAM_ONE_WAVE_KV: K V up to this runs one wave per utterance
CTC_BEAM_LDS_ENTRIES = 4096      # ASR_CTC_BEAM_LDS_ENTRIES: an utterance's T K history entries stay in LDS up to this count


def ctc_beam_ws_bytes(B, T, V, K):
    """asr_ctc_beam_ws_bytes on plain integers (no tensors, no GPU) -> the workspace bytes of a ctc_beam call;
    UnsupportedShape for sizes the kernel refuses (V < 2, a beam width outside 1 .. BEAM_KMAX)."""
    need = c_i64(0)
    rc = load().asr_ctc_beam_ws_bytes(int(B), int(T), int(V), int(K), ctypes.byref(need))
    if rc == -2:
        raise UnsupportedShape("ctc_beam: B %d, T %d, V %d, beam %d (beam 1 .. %d, V >= 2)" % (B, T, V, K, BEAM_KMAX))
    check(rc, "asr_ctc_beam_ws_bytes")
    return need.value


def ctc_beam(logits, frame_lens, K, hyp, hyp_len, score, ws):
    """asr_ctc_beam_f32 (csrc/ctc_beam.hip): the CTC prefix beam search of every utterance.  logits [B, T, V]
    fp32 raw (a view with row stride >= V is taken as it is), frame_lens int32 [B] on the device; the outputs hyp int32
    [B, K, T] (padded with -1), hyp_len int32 [B, K] (-1: an unused slot), score fp32 [B, K] (descending, -inf: unused) and
    the workspace ws (a float32 tensor of at least ctc_beam_ws_bytes bytes) are the caller's.  Two launches."""
    logits, ld = _ctc_view(logits, "ctc logits")
    B, T, V = logits.shape
    need = ctc_beam_ws_bytes(B, T, V, K)
    if ws.numel() * 4 < need or tuple(hyp.shape) != (B, K, T) or hyp_len.numel() != B * K or score.numel() != B * K:
        raise RuntimeError("ctc_beam: the workspace or an output is smaller than B %d, T %d, beam %d need" % (B, T, K))
    if not (hyp.is_contiguous() and hyp_len.is_contiguous() and score.is_contiguous()):
        raise RuntimeError("ctc_beam: the outputs must be contiguous")
    rc = load().asr_ctc_beam_f32(B, T, V, int(K), ptr(logits), int(ld), ptr(frame_lens), ptr(hyp), ptr(hyp_len), ptr(score),
                                 ptr(ws), stream())
    check(rc, "asr_ctc_beam_f32")
    LAUNCHES["ctc_beam"] += 1
    LAUNCHES["ctc_beam_launch"] += 2


def _ngram_table(table, V, what):
    """The device form of an n-gram LM (ngram.NgramTable after .to(device)): logp fp32 [S, V], nxt int32 [S, V], contiguous."""
    logp, nxt = table.logp, table.nxt
    if not (isinstance(logp, torch.Tensor) and logp.is_cuda and nxt.is_cuda):
        raise RuntimeError("%s: the n-gram table is not on the device (NgramLM.to(device))" % what)
    if logp.dtype != torch.float32 or nxt.dtype != torch.int32 or logp.shape != nxt.shape or logp.dim() != 2 or \
            not (logp.is_contiguous() and nxt.is_contiguous()):
        raise RuntimeError("%s: the n-gram table must be contiguous fp32 / int32 [S, V]" % what)
    if logp.shape[1] != V:
        raise UnsupportedShape("%s: the n-gram LM predicts %d tokens, the sequences are over %d" % (what, logp.shape[1], V))
    return logp, nxt, int(logp.shape[0])


def ngram_score(table, ids, lens, score, tok_score=None, eos_term=True):
    """asr_ngram_score_f32 (csrc/ngram.hip): the n-gram LM's log-probability of N padded id sequences.  table:
    the LM on the device; ids int32 [N, L] (a view with row stride >= L is taken as it is), lens int32 [N] (-1: an unused
    slot, -inf), both on the device; score fp32 [N] and tok_score (fp32 [N, L] or None) are the caller's.  One launch."""
    if ids.dim() != 2 or ids.dtype != torch.int32 or ids.stride(1) != 1 or lens.dtype != torch.int32:
        raise RuntimeError("ngram_score: ids must be int32 [N, L] with unit column stride, lens int32")
    N, L = ids.shape
    logp, nxt, S = _ngram_table(table, table.V, "ngram_score")
    if lens.numel() != N or score.numel() != N or not (lens.is_contiguous() and score.is_contiguous()) or \
            score.dtype != torch.float32:
        raise RuntimeError("ngram_score: lens and score must be contiguous with %d elements" % N)
    if tok_score is not None and (tuple(tok_score.shape) != (N, L) or not tok_score.is_contiguous() or
                                  tok_score.dtype != torch.float32):
        raise RuntimeError("ngram_score: tok_score must be contiguous fp32 [%d, %d]" % (N, L))
    rc = load().asr_ngram_score_f32(N, L, S, table.V, ptr(logp), ptr(nxt), int(table.start), int(table.eos) if eos_term else -1,
                                    ptr(ids), int(ids.stride(0)), ptr(lens), ptr(score),
                                    ptr(tok_score) if tok_score is not None else None, stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("ngram_score: %d states x %d tokens, start %d, eos %d" % (S, table.V, table.start, table.eos))
    check(rc, "asr_ngram_score_f32")
    LAUNCHES["ngram_score"] += 1


def ctc_beam_lm(logits, frame_lens, K, table, alpha, beta, eos_term, hyp, hyp_len, score, ctc_score, lm_score, ws):
    """asr_ctc_beam_lm_f32 (csrc/ctc_beam.hip): ctc_beam with the n-gram LM `table` (on the device) inside the
    search - candidates rank by (tot + alpha lm) + beta len.  The arguments and outputs of ctc_beam, and ctc_score / lm_score
    fp32 [B, K]: the CTC log-mass and the LM's sum (with the end term when eos_term) of every hypothesis; score is the
    rank.  Two launches."""
    logits, ld = _ctc_view(logits, "ctc logits")
    B, T, V = logits.shape
    logp, nxt, S = _ngram_table(table, V, "ctc_beam_lm")
    need = ctc_beam_ws_bytes(B, T, V, K)
    outs = (hyp_len, score, ctc_score, lm_score)
    if ws.numel() * 4 < need or tuple(hyp.shape) != (B, K, T) or any(o.numel() != B * K for o in outs):
        raise RuntimeError("ctc_beam_lm: the workspace or an output is smaller than B %d, T %d, beam %d need" % (B, T, K))
    if not (hyp.is_contiguous() and all(o.is_contiguous() for o in outs)):
        raise RuntimeError("ctc_beam_lm: the outputs must be contiguous")
    rc = load().asr_ctc_beam_lm_f32(B, T, V, int(K), ptr(logits), int(ld), ptr(frame_lens), S, ptr(logp), ptr(nxt),
                                    int(table.start), int(table.eos) if eos_term else -1, float(alpha), float(beta), ptr(hyp),
                                    ptr(hyp_len), ptr(score), ptr(ctc_score), ptr(lm_score), ptr(ws), stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("ctc_beam_lm: %d states x %d tokens, start %d, eos %d" % (S, V, table.start, table.eos))
    check(rc, "asr_ctc_beam_lm_f32")
    LAUNCHES["ctc_beam_lm"] += 1
    LAUNCHES["ctc_beam_lm_launch"] += 2


_WORD_LM_DTYPES = dict(trie_next=torch.int32, trie_word=torch.int32, arc_off=torch.int32, arc_word=torch.int32,
                       arc_logp=torch.float32, arc_next=torch.int32, bo_logp=torch.float32, bo_state=torch.int32,
                       uni_logp=torch.float32, uni_next=torch.int32)


def _word_lm_table(table, what):
    """The device form of a word LM (word_lm.WordTable after .to(device)) -> asr_word_lm_t; the tensors stay the table's."""
    t = WordLmTable()
    for name, dtype in _WORD_LM_DTYPES.items():
        a = getattr(table, name)
        if not (isinstance(a, torch.Tensor) and a.is_cuda):
            raise RuntimeError("%s: the word LM's tables are not on the device (WordLM.to(device))" % what)
        if a.dtype != dtype or not a.is_contiguous() or a.numel() == 0:
            raise RuntimeError("%s: the word LM's %s must be a contiguous, non-empty %s tensor" % (what, name, dtype))
        setattr(t, name, ptr(a))
    shapes = dict(trie_next=table.N * table.V, trie_word=table.N, arc_off=table.S + 1, arc_word=max(table.A, 1),
                  arc_logp=max(table.A, 1), arc_next=max(table.A, 1), bo_logp=table.S, bo_state=table.S, uni_logp=table.W,
                  uni_next=table.W)
    for name, n in shapes.items():
        if getattr(table, name).numel() != n:
            raise RuntimeError("%s: the word LM's %s holds %d elements, its sizes say %d" % (what, name, getattr(table, name).numel(), n))
    t.V, t.N, t.S, t.W, t.A = table.V, table.N, table.S, table.W, table.A
    t.space, t.start, t.empty, t.eos, t.unk = table.space, table.start, table.empty, table.eos, table.unk
    return t


def word_lm_score(table, ids, lens, score, n_words, word_score=None, eos_term=True):
    """asr_word_lm_score_f32 (csrc/word_lm.hip): the word LM's log-probability of N padded TOKEN id rows.
    table: the LM on the device; ids int32 [N, L] (a view with row stride >= L is taken as it is), lens int32 [N] (-1: an
    unused slot, -inf); score fp32 [N], n_words int32 [N] and word_score (fp32 [N, L] or None) are the caller's.  One launch."""
    if ids.dim() != 2 or ids.dtype != torch.int32 or ids.stride(1) != 1 or lens.dtype != torch.int32:
        raise RuntimeError("word_lm_score: ids must be int32 [N, L] with unit column stride, lens int32")
    N, L = ids.shape
    t = _word_lm_table(table, "word_lm_score")
    if lens.numel() != N or score.numel() != N or n_words.numel() != N or score.dtype != torch.float32 or \
            n_words.dtype != torch.int32 or not (lens.is_contiguous() and score.is_contiguous() and n_words.is_contiguous()):
        raise RuntimeError("word_lm_score: lens, score and n_words must be contiguous with %d elements" % N)
    if word_score is not None and (tuple(word_score.shape) != (N, L) or not word_score.is_contiguous() or
                                   word_score.dtype != torch.float32):
        raise RuntimeError("word_lm_score: word_score must be contiguous fp32 [%d, %d]" % (N, L))
    rc = load().asr_word_lm_score_f32(N, L, ctypes.byref(t), 1 if eos_term else 0, ptr(ids), int(ids.stride(0)), ptr(lens),
                                      ptr(score), ptr(n_words), ptr(word_score) if word_score is not None else None, stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("word_lm_score: a table of %d x %d trie entries, %d states, %d words" % (t.N, t.V, t.S, t.W))
    check(rc, "asr_word_lm_score_f32")
    LAUNCHES["word_lm_score"] += 1


def ctc_beam_wlm(logits, frame_lens, K, table, alpha, beta, eos_term, lexicon_only, hyp, hyp_len, score, ctc_score, lm_score,
                 n_words, ws):
    """asr_ctc_beam_wlm_f32 (csrc/ctc_beam.hip): ctc_beam with the lexicon and the word LM `table` (on the
    device) inside the search - candidates rank by (tot + alpha lm) + beta n_words.  The arguments and outputs of
    ctc_beam_lm, and n_words int32 [B, K].  Two launches."""
    logits, ld = _ctc_view(logits, "ctc logits")
    B, T, V = logits.shape
    if table.V != V:
        raise UnsupportedShape("ctc_beam_wlm: the word LM spells in %d tokens, the logits are over %d" % (table.V, V))
    t = _word_lm_table(table, "ctc_beam_wlm")
    need = ctc_beam_ws_bytes(B, T, V, K)
    outs = (hyp_len, score, ctc_score, lm_score, n_words)
    if ws.numel() * 4 < need or tuple(hyp.shape) != (B, K, T) or any(o.numel() != B * K for o in outs):
        raise RuntimeError("ctc_beam_wlm: the workspace or an output is smaller than B %d, T %d, beam %d need" % (B, T, K))
    if not (hyp.is_contiguous() and all(o.is_contiguous() for o in outs)):
        raise RuntimeError("ctc_beam_wlm: the outputs must be contiguous")
    rc = load().asr_ctc_beam_wlm_f32(B, T, V, int(K), ptr(logits), int(ld), ptr(frame_lens), ctypes.byref(t), float(alpha),
                                     float(beta), 1 if eos_term else 0, 1 if lexicon_only else 0, ptr(hyp), ptr(hyp_len),
                                     ptr(score), ptr(ctc_score), ptr(lm_score), ptr(n_words), ptr(ws), stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("ctc_beam_wlm: B %d, T %d, V %d, beam %d, a word LM over %d tokens" % (B, T, V, K, table.V))
    check(rc, "asr_ctc_beam_wlm_f32")
    LAUNCHES["ctc_beam_wlm"] += 1
    LAUNCHES["ctc_beam_wlm_launch"] += 2


_CONTEXT_DTYPES = dict(arc_off=torch.int32, arc_tok=torch.int32, arc_next=torch.int32, drow=torch.int32, dflt=torch.int32,
                       credit=torch.float32, pending=torch.float32, root=torch.int32)


def _context_table(table, rows, what, graph_of=None):
    """The device form of a context (context.ContextTable after .to(device)) -> (asr_context_t, graph_of int32 [rows] on the
    device: the caller's, or the table's own); the tensors stay the table's."""
    t = ContextTable()
    for name, dtype in _CONTEXT_DTYPES.items():
        a = getattr(table, name)
        if not (isinstance(a, torch.Tensor) and a.is_cuda):
            raise RuntimeError("%s: the context's tables are not on the device (ContextGraph.to(device))" % what)
        if a.dtype != dtype or not a.is_contiguous() or a.numel() == 0:
            raise RuntimeError("%s: the context's %s must be a contiguous, non-empty %s tensor" % (what, name, dtype))
        setattr(t, name, ptr(a))
    shapes = dict(arc_off=table.N + 1, arc_tok=max(table.A, 1), arc_next=max(table.A, 1), drow=table.N, dflt=table.R * table.V,
                  credit=table.N, pending=table.N, root=table.G)
    for name, n in shapes.items():
        if getattr(table, name).numel() != n:
            raise RuntimeError("%s: the context's %s holds %d elements, its sizes say %d" % (what, name, getattr(table, name).numel(), n))
    t.V, t.N, t.G, t.R, t.A = table.V, table.N, table.G, table.R, table.A
    if graph_of is None:
        graph_of = table.rows(rows)
    if not (graph_of.is_cuda and graph_of.dtype == torch.int32 and graph_of.is_contiguous() and graph_of.numel() == rows):
        raise RuntimeError("%s: graph_of must be a contiguous int32 tensor of %d rows on the device" % (what, rows))
    return t, graph_of


def context_score(table, ids, lens, score, tok_score=None, graph_of=None):
    """asr_context_score_f32 (csrc/context.hip): the bias of N padded TOKEN id rows under their context graphs.
    table: the context on the device; ids int32 [N, L] (a view with row stride >= L is taken as it is), lens int32 [N] (-1: an
    unused slot, -inf); graph_of int32 [N] on the device (None: the table's own, one per row); score fp32 [N] and tok_score
    (fp32 [N, L] or None) are the caller's.  One launch."""
    if ids.dim() != 2 or ids.dtype != torch.int32 or ids.stride(1) != 1 or lens.dtype != torch.int32:
        raise RuntimeError("context_score: ids must be int32 [N, L] with unit column stride, lens int32")
    N, L = ids.shape
    t, graph_of = _context_table(table, N, "context_score", graph_of)
    if lens.numel() != N or score.numel() != N or not (lens.is_contiguous() and score.is_contiguous()) or \
            score.dtype != torch.float32:
        raise RuntimeError("context_score: lens and score must be contiguous with %d elements" % N)
    if tok_score is not None and (tuple(tok_score.shape) != (N, L) or not tok_score.is_contiguous() or
                                  tok_score.dtype != torch.float32):
        raise RuntimeError("context_score: tok_score must be contiguous fp32 [%d, %d]" % (N, L))
    rc = load().asr_context_score_f32(N, L, ctypes.byref(t), ptr(graph_of), ptr(ids), int(ids.stride(0)), ptr(lens), ptr(score),
                                      ptr(tok_score) if tok_score is not None else None, stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("context_score: a context of %d states, %d graphs, %d rows x %d tokens" % (t.N, t.G, t.R, t.V))
    check(rc, "asr_context_score_f32")
    LAUNCHES["context_score"] += 1


def ctc_beam_ctx(logits, frame_lens, K, context, ctx_weight, table, alpha, beta, eos_term, hyp, hyp_len, score, ctc_score,
                 lm_score, ctx_score, ws):
    """asr_ctc_beam_ctx_f32 (csrc/ctc_beam.hip): ctc_beam (table None; lm_score None) or ctc_beam_lm (table: the
    n-gram LM on the device) with the context `context` (context.ContextTable on the device, one graph per utterance) inside
    the search - a candidate ranks by its rank without a context plus ctx_weight bias.  The arguments and outputs of
    ctc_beam_lm, and ctx_score fp32 [B, K]: the bias of every hypothesis.  Two launches."""
    logits, ld = _ctc_view(logits, "ctc logits")
    B, T, V = logits.shape
    if context.V != V:
        raise UnsupportedShape("ctc_beam_ctx: the context is over %d tokens, the logits are over %d" % (context.V, V))
    t, graph_of = _context_table(context, B, "ctc_beam_ctx")
    logp = nxt = None
    S = 0
    if table is not None:
        logp, nxt, S = _ngram_table(table, V, "ctc_beam_ctx")
    need = ctc_beam_ws_bytes(B, T, V, K)
    outs = (hyp_len, score, ctc_score, ctx_score) + ((lm_score,) if table is not None else ())
    if ws.numel() * 4 < need or tuple(hyp.shape) != (B, K, T) or any(o.numel() != B * K for o in outs):
        raise RuntimeError("ctc_beam_ctx: the workspace or an output is smaller than B %d, T %d, beam %d need" % (B, T, K))
    if not (hyp.is_contiguous() and all(o.is_contiguous() for o in outs)):
        raise RuntimeError("ctc_beam_ctx: the outputs must be contiguous")
    rc = load().asr_ctc_beam_ctx_f32(B, T, V, int(K), ptr(logits), int(ld), ptr(frame_lens), ctypes.byref(t), ptr(graph_of),
                                     float(ctx_weight), S, ptr(logp) if S else None, ptr(nxt) if S else None,
                                     int(table.start) if S else 0, int(table.eos) if S and eos_term else -1, float(alpha),
                                     float(beta), ptr(hyp), ptr(hyp_len), ptr(score), ptr(ctc_score),
                                     ptr(lm_score) if S else None, ptr(ctx_score), ptr(ws), stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("ctc_beam_ctx: B %d, T %d, V %d, beam %d, a context over %d tokens, %d LM states" % (B, T, V, K, context.V, S))
    check(rc, "asr_ctc_beam_ctx_f32")
    LAUNCHES["ctc_beam_ctx"] += 1
    LAUNCHES["ctc_beam_ctx_launch"] += 2


# ---------------------------------------------------------------------------------------------------------------------
# The front end (csrc/frontend.hip): waveforms -> features.
FBANK_FRAME_TILE = 8       # ASR_FBANK_FRAME_TILE
FBANK_MAX_MELS = 128       # ASR_FBANK_MAX_MELS
SAMPLES_I16, SAMPLES_F32 = 0, 1
CMVN_NONE, CMVN_GLOBAL, CMVN_UTTERANCE = 0, 1, 2


def fbank_num_frames(n_samples, frame_length, frame_shift):
    """asr_fbank_num_frames on plain integers (no tensors, no GPU): Kaldi's snip-edges frame count."""
    out = c_i64(0)
    check(load().asr_fbank_num_frames(int(n_samples), int(frame_length), int(frame_shift), ctypes.byref(out)),
          "asr_fbank_num_frames")
    return int(out.value)


def fbank_plan_bytes(n_fft):
    """asr_fbank_plan_bytes (no GPU); UnsupportedShape for an n_fft the kernel has no instantiation for."""
    out = c_i64(0)
    rc = load().asr_fbank_plan_bytes(int(n_fft), ctypes.byref(out))
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("fbank: n_fft %d (256 or 512)" % n_fft)
    check(rc, "asr_fbank_plan_bytes")
    return int(out.value)


def _mel(f):
    import numpy as np
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


class FbankPlan(object):
    """The geometry of asr_fbank_f32 and its tables (window, twiddles, mel weights: float64 on the host, rounded to fp32, in
    the layout include/asr_hip.h gives).  `words` is the host image (no GPU needed); `on(device)` is its device copy, made
    once per device.  high_freq <= 0 counts from the Nyquist frequency, as in Kaldi."""

    def __init__(self, sample_rate=16000, frame_length=400, frame_shift=160, n_fft=512, n_mels=80, low_freq=20.0,
                 high_freq=0.0, preemph=0.97):
        import numpy as np
        self.sample_rate, self.frame_length, self.frame_shift = int(sample_rate), int(frame_length), int(frame_shift)
        self.n_fft, self.n_mels, self.preemph = int(n_fft), int(n_mels), float(preemph)
        nyquist = 0.5 * self.sample_rate
        self.low_freq = float(low_freq)
        self.high_freq = float(high_freq) if high_freq and high_freq > 0 else nyquist + float(high_freq or 0.0)
        if (self.n_fft not in (256, 512) or not 0 < self.frame_length <= self.n_fft or self.frame_shift <= 0
                or not 1 <= self.n_mels <= FBANK_MAX_MELS):
            raise UnsupportedShape("fbank: n_fft %d (256 or 512), frame length %d (<= n_fft), shift %d, %d mel bins (1 .. %d)"
                                   % (self.n_fft, self.frame_length, self.frame_shift, self.n_mels, FBANK_MAX_MELS))
        if not 0.0 <= self.low_freq < self.high_freq <= nyquist:
            raise ValueError("fbank: need 0 <= low_freq < high_freq <= Nyquist, got %g, %g" % (self.low_freq, self.high_freq))
        N, M, L = self.n_fft, self.n_fft // 2, self.frame_length
        window = np.zeros(N)
        window[:L] = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L) / max(L - 1, 1))) ** 0.85
        a = 2.0 * np.pi * np.arange(M // 2) / M
        tw = np.stack([np.cos(a), -np.sin(a)], 1).reshape(-1)
        a = 2.0 * np.pi * np.arange(M) / N
        ut = np.stack([np.cos(a), -np.sin(a)], 1).reshape(-1)
        edges = _mel(self.low_freq) + (_mel(self.high_freq) - _mel(self.low_freq)) * np.arange(self.n_mels + 2) / (self.n_mels + 1)
        mel_bins = _mel(np.arange(M) * (self.sample_rate / float(N)))
        start = np.zeros(FBANK_MAX_MELS, np.int32)
        length = np.zeros(FBANK_MAX_MELS, np.int32)
        woff = np.zeros(FBANK_MAX_MELS, np.int32)
        packed = np.zeros(N)
        used = 0
        for j in range(self.n_mels):
            left, centre, right = edges[j], edges[j + 1], edges[j + 2]
            up = (mel_bins - left) / (centre - left)
            down = (right - mel_bins) / (right - centre)
            w = np.where((mel_bins > left) & (mel_bins < right), np.where(mel_bins <= centre, up, down), 0.0)
            nz = np.nonzero(w)[0]
            if nz.size:
                start[j], length[j], woff[j] = nz[0], nz[-1] - nz[0] + 1, used
                packed[used:used + length[j]] = w[nz[0]:nz[-1] + 1]
                used += int(length[j])
        assert used <= N
        self.words = np.concatenate([window.astype(np.float32).view(np.int32), tw.astype(np.float32).view(np.int32),
                                     ut.astype(np.float32).view(np.int32), start, length, woff,
                                     packed.astype(np.float32).view(np.int32)])
        assert self.words.size * 4 == fbank_plan_bytes(N)
        self._dev = {}

    def num_frames(self, n_samples):
        n = int(n_samples)
        return 1 + (n - self.frame_length) // self.frame_shift if n >= self.frame_length else 0

    def on(self, device):
        key = str(torch.device(device))
        buf = self._dev.get(key)
        if buf is None:
            buf = self._dev[key] = torch.from_numpy(self.words).to(device)
        return buf


def fbank(plan, samples, offsets, T_max, out, col0=0, use_log=True):
    """asr_fbank_f32: samples = ONE packed 1-D int16 or float32 tensor, offsets int64 [B + 1] on the device -> rows (b, t) of
    out [B, T_max, ld] at columns col0 .. col0 + n_mels (rows behind an utterance's frames are not touched)."""
    if not (samples.is_cuda and offsets.is_cuda and out.is_cuda):
        raise RuntimeError("fbank: tensors must live on the GPU: the HIP path has no CPU fallback")
    if samples.dtype not in (torch.int16, torch.float32) or samples.dim() != 1 or not samples.is_contiguous():
        raise RuntimeError("fbank: samples must be one packed 1-D int16 or float32 tensor")
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous() or offsets.numel() < 2:
        raise RuntimeError("fbank: offsets must be int64 [B + 1]")
    B = offsets.numel() - 1
    if out.dtype != torch.float32 or out.dim() != 3 or out.shape[0] != B or out.shape[1] != T_max or out.stride(2) != 1 \
            or out.stride(0) != T_max * out.stride(1):
        raise RuntimeError("fbank: out must be float32 [B, T_max, ld] with rows of one leading dimension")
    rc = load().asr_fbank_f32(B, int(T_max), c_p(samples.data_ptr()), SAMPLES_I16 if samples.dtype == torch.int16 else SAMPLES_F32,
                              c_p(offsets.data_ptr()), plan.frame_length, plan.frame_shift, plan.n_fft, plan.n_mels,
                              plan.preemph, 1 if use_log else 0, c_p(plan.on(out.device).data_ptr()), ptr(out),
                              int(out.stride(1)), int(col0), stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("fbank: B %d, n_fft %d, frame length %d, %d mel bins" % (B, plan.n_fft, plan.frame_length, plan.n_mels))
    check(rc, "asr_fbank_f32")
    LAUNCHES["fbank"] += 1
    return out


def feat_cmvn_stats(x, n_mels, frame_lens, stats):
    """asr_feat_cmvn_stats_f32: x [B, T, ld >= n_mels], frame_lens int32 [B] -> stats [B, 2, n_mels] (mean, 1 / std)."""
    B, T = int(x.shape[0]), int(x.shape[1])
    rc = load().asr_feat_cmvn_stats_f32(B, T, int(n_mels), ptr(x), int(x.stride(1)), ptr(frame_lens), ptr(stats), stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("feat_cmvn_stats: %d bins (at most %d)" % (n_mels, FBANK_MAX_MELS))
    check(rc, "asr_feat_cmvn_stats_f32")
    LAUNCHES["feat_cmvn_stats"] += 1
    return stats


def feat_finish(x, n_mels, frame_lens, out, order=0, cmvn=CMVN_NONE, stats=None, masks=None, n_freq_masks=0, n_time_masks=0):
    """asr_feat_finish_f32: static features x [B, T, ld >= n_mels] -> out [B, T, n_mels (1 + order)]: CMVN, deltas, masks
    (int32 [B, n_freq_masks + n_time_masks, 2] of (start, width)), zeros behind every utterance."""
    B, T = int(x.shape[0]), int(x.shape[1])
    if tuple(out.shape) != (B, T, n_mels * (1 + order)) or not out.is_contiguous() or x.stride(2) != 1 \
            or x.stride(0) != T * x.stride(1):
        raise RuntimeError("feat_finish: out must be contiguous [B, T, n_mels (1 + order)], x [B, T, ld]")
    if masks is not None and (masks.dtype != torch.int32 or tuple(masks.shape) != (B, n_freq_masks + n_time_masks, 2)
                              or not masks.is_contiguous()):
        raise RuntimeError("feat_finish: masks must be int32 [B, n_freq_masks + n_time_masks, 2]")
    rc = load().asr_feat_finish_f32(B, T, int(n_mels), int(order), ptr(x), int(x.stride(1)), ptr(frame_lens), int(cmvn),
                                    ptr(stats), ptr(masks), int(n_freq_masks), int(n_time_masks), ptr(out), stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("feat_finish: %d bins (at most %d), delta order %d (0 .. 2)" % (n_mels, FBANK_MAX_MELS, order))
    check(rc, "asr_feat_finish_f32")
    LAUNCHES["feat_finish"] += 1
    return out

# ---------------------------------------------------------------------------------------------------------------------
# Speed perturbation (csrc/resample.hip): a polyphase resampler in front of the fbank.
RESAMPLE_TILE = 1024          # ASR_RESAMPLE_TILE: output samples per workgroup
RESAMPLE_MAX_FACTORS = 8      # ASR_RESAMPLE_MAX_FACTORS
RESAMPLE_MAX_PHASES = 32      # ASR_RESAMPLE_MAX_PHASES
RESAMPLE_MAX_TAPS = 64        # ASR_RESAMPLE_MAX_TAPS
RESAMPLE_MAX_SPAN = 2176      # ASR_RESAMPLE_MAX_SPAN
RESAMPLE_LPW, RESAMPLE_ROLLOFF = 6, 0.99


def resample_plan_bytes(geometry):
    """asr_resample_plan_bytes (no GPU) on an int32 [F, 5] array of (orig, new, width, taps, table offset); UnsupportedShape
    beyond the header's limits."""
    import numpy as np
    g = np.ascontiguousarray(geometry, dtype=np.int32).reshape(-1, 5)
    out = c_i64(0)
    rc = load().asr_resample_plan_bytes(int(g.shape[0]), c_p(g.ctypes.data), ctypes.byref(out))
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("resample: %d factors (at most %d), phases %s (at most %d), taps %s (at most %d), speed at most 2"
                               % (g.shape[0], RESAMPLE_MAX_FACTORS, g[:, 1].tolist(), RESAMPLE_MAX_PHASES, g[:, 3].tolist(),
                                  RESAMPLE_MAX_TAPS))
    check(rc, "asr_resample_plan_bytes")
    return int(out.value)


class ResamplePlan(object):
    """The polyphase banks of asr_resample_f32 for a list of speed factors at one sample rate (include/asr_hip.h gives the
    definition): factor s resamples from orig = round(s sample_rate) to new = sample_rate, both over their gcd.  The taps
    are computed in float64 here and rounded to fp32 once.  `geometry` int32 [F, 5] = (orig, new, width, taps, table offset),
    `tables` the fp32 host image (no GPU needed); `on(device)` is its device copy, made once per device."""

    def __init__(self, sample_rate, factors):
        import math
        import numpy as np
        self.sample_rate, self.factors = int(sample_rate), [float(s) for s in factors]
        if self.sample_rate <= 0 or not self.factors or min(self.factors) <= 0:
            raise ValueError("resample: need a positive sample rate and positive speed factors, got %d, %s"
                             % (self.sample_rate, self.factors))
        if len(self.factors) > RESAMPLE_MAX_FACTORS:
            raise UnsupportedShape("resample: %d factors (at most %d)" % (len(self.factors), RESAMPLE_MAX_FACTORS))
        geometry, banks, used = [], [], 0
        for s in self.factors:
            orig, new = int(round(s * self.sample_rate)), self.sample_rate
            g = math.gcd(orig, new)
            orig, new = orig // g, new // g
            base = min(orig, new) * RESAMPLE_ROLLOFF
            width = int(math.ceil(RESAMPLE_LPW * orig / base))
            taps = 2 * width + orig
            if new > RESAMPLE_MAX_PHASES or taps > RESAMPLE_MAX_TAPS:       # (before a table of that size is built)
                raise UnsupportedShape("resample: factor %g at %d Hz is %d / %d: %d phases (at most %d), %d taps (at most %d)"
                                       % (s, self.sample_rate, orig, new, new, RESAMPLE_MAX_PHASES, taps, RESAMPLE_MAX_TAPS))
            t = ((np.arange(taps, dtype=np.float64)[None, :] - width) / orig - np.arange(new, dtype=np.float64)[:, None] / new) * base
            t = np.clip(t, -RESAMPLE_LPW, RESAMPLE_LPW)
            window = np.cos(t * np.pi / RESAMPLE_LPW / 2.0) ** 2
            a = t * np.pi
            sinc = np.where(a == 0, 1.0, np.sin(a) / np.where(a == 0, 1.0, a))
            banks.append((sinc * window * (base / orig)).astype(np.float32))
            geometry.append((orig, new, width, taps, used))
            used += new * taps
        self.geometry = np.asarray(geometry, dtype=np.int32)
        self.tables = np.concatenate([b.reshape(-1) for b in banks])
        assert self.tables.size * 4 == resample_plan_bytes(self.geometry)
        self._dev = {}

    def __len__(self):
        return len(self.factors)

    def bank(self, f):
        """The fp32 taps [new, taps] of factor f (a view of the host image)."""
        orig, new, width, taps, off = (int(v) for v in self.geometry[f])
        return self.tables[off:off + new * taps].reshape(new, taps)

    def out_samples(self, n_samples, f):
        """ceil(new n / orig): the samples factor f makes of n (integer arithmetic)."""
        orig, new = int(self.geometry[f, 0]), int(self.geometry[f, 1])
        return -(-new * int(n_samples) // orig)

    def on(self, device):
        key = str(torch.device(device))
        buf = self._dev.get(key)
        if buf is None:
            buf = self._dev[key] = torch.from_numpy(self.tables).to(device)
        return buf


def resample(plan, samples, in_offsets, factor_index, out_offsets, out, max_out=None):
    """asr_resample_f32: samples = ONE packed 1-D int16 or float32 tensor, in_offsets / out_offsets int64 [B + 1] and
    factor_index int32 [B] on the device -> utterance b resampled by plan factor factor_index[b] at out[out_offsets[b] ..),
    `out` ONE packed 1-D float32 tensor.  factor_index may also be a host sequence: it is then checked against the plan
    (UnsupportedShape outside it) and uploaded; a device tensor is trusted, and the kernel clamps it into the plan.  max_out:
    the longest row's output length (default: out.numel(), an upper bound)."""
    if not (samples.is_cuda and in_offsets.is_cuda and out_offsets.is_cuda and out.is_cuda):
        raise RuntimeError("resample: tensors must live on the GPU: the HIP path has no CPU fallback")
    if samples.dtype not in (torch.int16, torch.float32) or samples.dim() != 1 or not samples.is_contiguous():
        raise RuntimeError("resample: samples must be one packed 1-D int16 or float32 tensor")
    B = in_offsets.numel() - 1
    for name, o in (("in_offsets", in_offsets), ("out_offsets", out_offsets)):
        if o.dtype != torch.int64 or o.dim() != 1 or not o.is_contiguous() or o.numel() != B + 1 or B < 1:
            raise RuntimeError("resample: %s must be int64 [B + 1]" % name)
    if out.dtype != torch.float32 or out.dim() != 1 or not out.is_contiguous():
        raise RuntimeError("resample: out must be one packed 1-D float32 tensor")
    if not torch.is_tensor(factor_index):
        import numpy as np
        fi = np.asarray(factor_index, dtype=np.int64).reshape(-1)
        if fi.size != B or (fi.size and (fi.min() < 0 or fi.max() >= len(plan))):
            raise UnsupportedShape("resample: factor indices %s for %d rows and a plan of %d factors" % (fi.tolist(), B, len(plan)))
        factor_index = to_device_i32(fi, out.device)
    if not factor_index.is_cuda or factor_index.dtype != torch.int32 or factor_index.numel() != B or not factor_index.is_contiguous():
        raise RuntimeError("resample: factor_index must be int32 [B] on the GPU (or a host sequence)")
    max_out = int(out.numel() if max_out is None else max_out)
    if max_out <= 0:
        return out
    tables = plan.on(out.device)
    rc = load().asr_resample_f32(B, max_out, c_p(samples.data_ptr()), SAMPLES_I16 if samples.dtype == torch.int16 else SAMPLES_F32,
                                 int(samples.numel()), c_p(in_offsets.data_ptr()), c_p(factor_index.data_ptr()),
                                 c_p(out_offsets.data_ptr()), len(plan), c_p(plan.geometry.ctypes.data),
                                 c_p(tables.data_ptr()), int(tables.numel()) * 4, ptr(out), int(out.numel()), stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("resample: B %d (at most 65535), %d factors" % (B, len(plan)))
    check(rc, "asr_resample_f32")
    LAUNCHES["resample"] += 1
    return out


# Reverberation and additive noise (csrc/augment.hip): two passes between the resampler and the fbank.
REVERB_TILE = 4096            # ASR_REVERB_TILE: output samples per workgroup
REVERB_CHUNK = 2048           # ASR_REVERB_CHUNK: taps staged in LDS at a time
REVERB_MAX_TAPS = 8192        # ASR_REVERB_MAX_TAPS
REVERB_PRE = 32               # taps kept in front of the direct path
NOISE_TILE = 4096             # ASR_NOISE_TILE: samples per power partial


def load_bank(bank):
    """An `.npz` path, or a dict, with `samples` (1-D int16 / float32) and `offsets` (int64 [n + 1]) -> the list of clips."""
    import numpy as np
    if isinstance(bank, (str, bytes, os.PathLike)):
        with np.load(bank) as z:
            samples, offsets = np.asarray(z["samples"]), np.asarray(z["offsets"])
    else:
        samples, offsets = np.asarray(bank["samples"]), np.asarray(bank["offsets"])
    offsets = offsets.astype(np.int64).reshape(-1)
    if samples.ndim != 1 or samples.dtype not in (np.int16, np.float32):
        raise ValueError("bank: `samples` must be 1-D int16 or float32, got %s %s" % (samples.dtype, samples.shape))
    if offsets.size < 2 or offsets[0] < 0 or offsets[-1] > samples.size or (np.diff(offsets) <= 0).any():
        raise ValueError("bank: `offsets` must be n + 1 ascending positions inside `samples`, no empty clip")
    return [samples[a:b] for a, b in zip(offsets[:-1], offsets[1:])]


class ReverbPlan(object):
    """The RIR bank of asr_reverb_f32, prepared on the host (no GPU needed): every RIR's direct path d is the first index of
    max |h|; the RIR is cut to [d - pre, d - pre + max_taps) with pre = min(d, REVERB_PRE) - a longer one is cut, not refused -
    scaled to unit energy in float64, rounded to fp32 once and packed.  (normalize=False keeps the taps' values and a larger
    `pre` keeps more of the head: the kernel takes any d in [0, taps); the tests use both.)  `geometry` int64 [n, 3] = (offset, taps, d after the cut), `bank` the fp32 host image; `on(device)` -> (bank,
    geometry) on the device, copied once per device."""

    def __init__(self, rirs, max_taps=4096, normalize=True, pre=REVERB_PRE):
        import numpy as np
        self.max_taps, keep = int(max_taps), int(pre)
        if not 1 <= self.max_taps <= REVERB_MAX_TAPS:
            raise UnsupportedShape("reverb: max_taps %d (1 .. %d)" % (self.max_taps, REVERB_MAX_TAPS))
        geometry, taps, used = [], [], 0
        for h in rirs:
            h = np.asarray(h, dtype=np.float64).reshape(-1)
            if h.size == 0 or not np.isfinite(h).all() or not np.abs(h).max() > 0:
                raise ValueError("reverb: an RIR must be finite and not all zero")
            d = int(np.argmax(np.abs(h)))                  # (argmax: the FIRST index of the maximum)
            pre = min(d, keep)
            h = h[d - pre:d - pre + self.max_taps]
            if normalize:
                h = h / np.sqrt((h * h).sum())
            taps.append(h.astype(np.float32))
            geometry.append((used, h.size, pre))
            used += h.size
        if not geometry:
            raise ValueError("reverb: an empty RIR bank")
        self.geometry = np.asarray(geometry, dtype=np.int64)
        self.bank = np.concatenate(taps)
        self._dev = {}

    def __len__(self):
        return int(self.geometry.shape[0])

    def rir(self, r):
        """-> (the fp32 taps of RIR r as the kernel reads them, d)"""
        off, n, d = (int(v) for v in self.geometry[r])
        return self.bank[off:off + n], d

    def on(self, device):
        key = str(torch.device(device))
        pair = self._dev.get(key)
        if pair is None:
            pair = self._dev[key] = (torch.from_numpy(self.bank).to(device), torch.from_numpy(self.geometry).to(device))
        return pair


class NoiseBank(object):
    """The clips of asr_noise_mix_f32, packed as fp32 with offsets (int16 clips are converted by value); `on(device)` ->
    (bank, offsets) on the device, copied once per device."""

    def __init__(self, clips):
        import numpy as np
        clips = [np.asarray(c).reshape(-1).astype(np.float32) for c in clips]
        if not clips or min(c.size for c in clips) == 0:
            raise ValueError("noise: an empty bank, or an empty clip")
        self.offsets = np.concatenate([[0], np.cumsum([c.size for c in clips])]).astype(np.int64)
        self.bank = np.concatenate(clips)
        self._dev = {}

    def __len__(self):
        return int(self.offsets.size - 1)

    def clip(self, c):
        return self.bank[int(self.offsets[c]):int(self.offsets[c + 1])]

    def clip_len(self, c):
        return int(self.offsets[c + 1] - self.offsets[c])

    def on(self, device):
        key = str(torch.device(device))
        pair = self._dev.get(key)
        if pair is None:
            pair = self._dev[key] = (torch.from_numpy(self.bank).to(device), torch.from_numpy(self.offsets).to(device))
        return pair


def _augment_args(name, samples, offsets, out):
    if not (samples.is_cuda and offsets.is_cuda and out.is_cuda):
        raise RuntimeError("%s: tensors must live on the GPU: the HIP path has no CPU fallback" % name)
    if samples.dtype not in (torch.int16, torch.float32) or samples.dim() != 1 or not samples.is_contiguous():
        raise RuntimeError("%s: samples must be one packed 1-D int16 or float32 tensor" % name)
    B = offsets.numel() - 1
    if offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous() or B < 1:
        raise RuntimeError("%s: offsets must be int64 [B + 1]" % name)
    if out.dtype != torch.float32 or out.dim() != 1 or not out.is_contiguous():
        raise RuntimeError("%s: out must be one packed 1-D float32 tensor" % name)
    return B


def _row_index(name, index, B, n, device):
    """A per-row index: a host sequence is checked against the bank (UnsupportedShape outside [-1, n)) and uploaded; a device
    tensor is trusted, and the kernel clamps it."""
    if not torch.is_tensor(index):
        import numpy as np
        idx = np.asarray(index, dtype=np.int64).reshape(-1)
        if idx.size != B or (idx.size and (idx.min() < -1 or idx.max() >= n)):
            raise UnsupportedShape("%s: indices %s for %d rows and a bank of %d" % (name, idx.tolist(), B, n))
        index = to_device_i32(idx, device)
    if not index.is_cuda or index.dtype != torch.int32 or index.numel() != B or not index.is_contiguous():
        raise RuntimeError("%s: the row indices must be int32 [B] on the GPU (or a host sequence)" % name)
    return index


def reverb(plan, samples, offsets, rir_index, out, max_len=None):
    """asr_reverb_f32: samples = ONE packed 1-D int16 or float32 tensor, offsets int64 [B + 1] on the device, rir_index int32
    [B] on the device or a host sequence (-1: the row is copied by value) -> every row convolved with its RIR of `plan`,
    undelayed, at the same offsets of `out` (ONE packed 1-D float32 tensor, not `samples`).  max_len: the longest row
    (default: out.numel(), an upper bound)."""
    B = _augment_args("reverb", samples, offsets, out)
    rir_index = _row_index("reverb", rir_index, B, len(plan), out.device)
    max_len = int(out.numel() if max_len is None else max_len)
    if max_len <= 0:
        return out
    bank, geometry = plan.on(out.device)
    rc = load().asr_reverb_f32(B, max_len, c_p(samples.data_ptr()), SAMPLES_I16 if samples.dtype == torch.int16 else SAMPLES_F32,
                               int(samples.numel()), c_p(offsets.data_ptr()), c_p(rir_index.data_ptr()), len(plan),
                               c_p(plan.geometry.ctypes.data), c_p(geometry.data_ptr()), c_p(bank.data_ptr()),
                               int(bank.numel()), ptr(out), int(out.numel()), stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("reverb: B %d (at most 65535), taps at most %d" % (B, REVERB_MAX_TAPS))
    check(rc, "asr_reverb_f32")
    LAUNCHES["reverb"] += 1
    return out


def noise_mix(noise_bank, samples, offsets, clip_index, start, scale, out=None, max_len=None, gains=None):
    """asr_noise_mix_f32: row b of the packed samples + g * its clip of `noise_bank` read cyclically from start[b], g =
    scale[b] sqrt(P_row / P_clip), scale = 10^(-snr_db / 20) from the host.  clip_index int32 [B] (-1: no clip), start int64
    [B], scale float32 [B]: device tensors or host sequences.  out: None mixes a float32 `samples` in place; gains: None or
    float32 [B] on the device, filled with g.  -> out."""
    out = samples if out is None else out
    B = _augment_args("noise_mix", samples, offsets, out)
    dev = out.device
    clip_index = _row_index("noise_mix", clip_index, B, len(noise_bank), dev)
    if not torch.is_tensor(start):
        start = to_device_i64(start, dev)
    if not torch.is_tensor(scale):
        scale = to_device_f32(scale, dev)
    if (not start.is_cuda or start.dtype != torch.int64 or start.numel() != B or not start.is_contiguous()
            or not scale.is_cuda or scale.dtype != torch.float32 or scale.numel() != B or not scale.is_contiguous()):
        raise RuntimeError("noise_mix: start must be int64 [B] and scale float32 [B] on the GPU (or host sequences)")
    if gains is not None and (not gains.is_cuda or gains.dtype != torch.float32 or gains.numel() != B or not gains.is_contiguous()):
        raise RuntimeError("noise_mix: gains must be float32 [B] on the GPU")
    if out.data_ptr() == samples.data_ptr() and samples.dtype != torch.float32:
        raise RuntimeError("noise_mix: int16 samples cannot be mixed in place")
    max_len = int(out.numel() if max_len is None else max_len)
    if max_len <= 0:
        return out
    bank, offs_d = noise_bank.on(dev)
    ws = torch.empty(2 * B * (-(-max_len // NOISE_TILE)), device=dev, dtype=torch.float64)
    rc = load().asr_noise_mix_f32(B, max_len, c_p(samples.data_ptr()), SAMPLES_I16 if samples.dtype == torch.int16 else SAMPLES_F32,
                                  int(samples.numel()), c_p(offsets.data_ptr()), c_p(clip_index.data_ptr()),
                                  c_p(start.data_ptr()), c_p(scale.data_ptr()), len(noise_bank),
                                  c_p(noise_bank.offsets.ctypes.data), c_p(offs_d.data_ptr()), c_p(bank.data_ptr()),
                                  int(bank.numel()), c_p(ws.data_ptr()), int(ws.numel()) * 8, ptr(out), int(out.numel()),
                                  c_p(gains.data_ptr()) if gains is not None else None, stream())
    if rc == ASR_E_SHAPE:
        raise UnsupportedShape("noise_mix: B %d (at most 65535)" % B)
    check(rc, "asr_noise_mix_f32")
    LAUNCHES["noise_mix"] += 1
    return out


def colsum(X, out=None, accumulate=False):
    X, ldx = _rowmajor(_dev(X, "X"))
    M, N = X.shape
    if out is None:
        out = torch.empty(N, device=X.device, dtype=torch.float32)
    if DETERMINISTIC[0]:
        ws, nbytes = det_workspace(X.device, ((M + 255) // 256) * N * 4 if M > 256 else 0)
        check(load().asr_colsum_det_f32(M, N, ptr(X), ldx, ptr(out), int(accumulate), ws, nbytes, stream()), "asr_colsum_det_f32")
        return out
    check(load().asr_colsum_f32(M, N, ptr(X), ldx, ptr(out), int(accumulate), stream()), "asr_colsum_f32")
    return out


_pinned_ring = {}
_upload_streams = {}
# The side stream costs the host ~25 us per upload (stream switch, event record / wait): worth it when the GPU is the
# bottleneck (the copy leaves the compute stream), a loss when the host is (cfg-1: 2.01 -> 2.32 ms per step).  E2E.forward
# switches it on for batches of at least UPLOAD_SIDE_MIN_FRAMES padded frames (B * T); ASR_UPLOAD_STREAM=0/1 forces it.
UPLOAD_SIDE_STREAM = [os.environ.get("ASR_UPLOAD_STREAM", "0") == "1"]
UPLOAD_SIDE_MIN_FRAMES = 4096


def upload_side_stream_for(n_frames):
    if "ASR_UPLOAD_STREAM" not in os.environ:
        UPLOAD_SIDE_STREAM[0] = int(n_frames) >= UPLOAD_SIDE_MIN_FRAMES


RING_SLOTS = 8


def _ring_event():
    """The event behind a lap's copies (no timing: the cheap kind)."""
    return torch.cuda.Event()


def _ring_buffer(size, torch_dtype):
    return torch.empty(size, dtype=torch_dtype).pin_memory()


def _ring_new(size, torch_dtype):
    return dict(bufs=[_ring_buffer(size, torch_dtype) for _ in range(RING_SLOTS)], i=0, stream=None, open=False, lap=[],
                pending=[], retired=[])


def _ring_stage(ring, flat):
    """Next slot of `ring`, filled with the host tensor `flat` -> slot index.  The slot's buffer was the source of an
    asynchronous copy RING_SLOTS uploads ago, and a copy reads its pinned source when it RUNS: the buffer is rewritten only
    once that copy is known to have run.  One event per lap of the ring says so (_ring_sent records it behind the lap's last
    copy): at the start of a lap the events of the lap before are looked at once, and in the steady state they have fired
    long ago - the other seven uploads of the lap cost nothing.  With a GPU that lags further behind (a pipelined step, a
    long kernel in front) the host does NOT wait: while an event is outstanding, every slot it comes to retires its buffer
    (kept alive until those events have fired) and takes a fresh one."""
    k = ring["i"] % RING_SLOTS
    ring["i"] += 1
    if k == 0 and ring["lap"]:
        ring["pending"], ring["lap"] = ring["pending"] + ring["lap"], []
    if ring["pending"]:
        ring["pending"] = [e for e in ring["pending"] if not e.query()]
        if ring["pending"]:
            ring["retired"] = [(b, evs) for b, evs in ring["retired"] if not all(e.query() for e in evs)]
            ring["retired"].append((ring["bufs"][k], list(ring["pending"])))
            ring["bufs"][k] = _ring_buffer(flat.numel(), flat.dtype)
        else:
            ring["retired"] = []            # (every event a retired buffer waited for was in `pending`)
    ring["bufs"][k].copy_(flat)
    return k


def _ring_sent(ring, k, stream):
    """The copy out of slot k has just been enqueued on `stream`.  The lap's event goes behind its last copy; a lap whose
    copies went to more than one stream (the upload stream switched on or off, another current stream) gets one per stream."""
    if ring["open"] and ring["stream"] != stream:
        ev = _ring_event()
        ev.record(ring["stream"])
        ring["lap"].append(ev)
    ring["stream"], ring["open"] = stream, True
    if k == RING_SLOTS - 1:
        ev = _ring_event()
        ev.record(stream)
        ring["lap"].append(ev)
        ring["open"] = False


def _to_device(arr, torch_dtype, device):
    """Host array -> device tensor without blocking the host and without a place in the compute stream: staged through a
    small ring of pinned buffers and copied on a side stream (the compute stream only waits for the copy's event - the
    host runs ahead of the GPU, so the copy has long finished when the stream gets there; as an in-stream copy each of
    these small uploads cost ~10 us of the step).  The tensor returned keeps its values whatever the host does next: every
    lap of the ring leaves an event behind its copies, on the stream that runs them, and a buffer is rewritten only after
    the events of the lap before have fired (_ring_stage); on the CPU the result owns its memory."""
    dev = torch.device(device)
    flat = torch.from_numpy(arr.reshape(-1))
    if dev.type != "cuda":      # (no copy engine, no ring: .to("cpu") of a host buffer is the buffer itself)
        return flat.to(torch_dtype, copy=True).view(arr.shape)
    key = (str(device), str(torch_dtype), arr.size)
    ring = _pinned_ring.get(key)
    if ring is None:            # (not setdefault(key, dict(...)): its default is built - eight pinned allocations - on EVERY call)
        ring = _pinned_ring[key] = _ring_new(arr.size, torch_dtype)
    k = _ring_stage(ring, flat)
    buf = ring["bufs"][k]
    main = torch.cuda.current_stream(dev)
    if not UPLOAD_SIDE_STREAM[0]:
        out = buf.to(dev, non_blocking=True)
        _ring_sent(ring, k, main)
        return out.view(arr.shape)
    side = _upload_streams.get(str(dev))
    if side is None:
        side = _upload_streams.setdefault(str(dev), torch.cuda.Stream(device=dev))
    with torch.cuda.stream(side):
        out = buf.to(dev, non_blocking=True)
    _ring_sent(ring, k, side)
    main.wait_stream(side)
    out.record_stream(main)
    return out.view(arr.shape)


def to_device_i32(values, device):
    """Host ints -> int32 device tensor (see _to_device)."""
    import numpy as np
    return _to_device(np.asarray(values, dtype=np.int32), torch.int32, device)


def to_device_i64(values, device):
    """Host ints -> int64 device tensor (index tensors: no conversion kernel on the device)."""
    import numpy as np
    return _to_device(np.asarray(values, dtype=np.int64), torch.int64, device)


def to_device_f32(array, device):
    """Host float32 array -> device tensor (see _to_device)."""
    import numpy as np
    return _to_device(np.ascontiguousarray(array, dtype=np.float32), torch.float32, device)


def _ptr_array(tensors):
    return (c_p * len(tensors))(*[_dev(t).data_ptr() for t in tensors])


def lstm_pack(params, ndir, w_ih_cat, w_hh_il, bias):
    """params: per direction (w_ih, w_hh, b_ih, b_hh) in torch layout -> interleaved kernel layout (one launch)."""
    H, I = params[1].shape[1], params[0].shape[1]
    ps = [p if p.is_contiguous() else p.contiguous() for p in params]
    check(load().asr_lstm_pack_f32(H, I, ndir, _ptr_array(ps[0::4]), _ptr_array(ps[1::4]), _ptr_array(ps[2::4]),
                                   _ptr_array(ps[3::4]), ptr(w_ih_cat), ptr(w_hh_il), ptr(bias), stream()),
          "asr_lstm_pack_f32")


def lstm_unpack(H, I, ndir, dw_ih_cat, dw_hh_il, db_il, two_biases=False):
    """Interleaved gradients -> [dw_ih, dw_hh, db] per direction in torch layout (one launch).  two_biases: also a second,
    independent copy of every bias gradient (for b_hh: autograd clones a tensor returned for two parameters)."""
    dev = dw_ih_cat.device
    f32 = dict(device=dev, dtype=torch.float32)
    dw_ih = [torch.empty(4 * H, I, **f32) for _ in range(ndir)]
    dw_hh = [torch.empty(4 * H, H, **f32) for _ in range(ndir)]
    db = [torch.empty(4 * H, **f32) for _ in range(ndir)]
    db2 = [torch.empty(4 * H, **f32) for _ in range(ndir)] if two_biases else None
    check(load().asr_lstm_unpack2_f32(H, I, ndir, ptr(dw_ih_cat), ptr(dw_hh_il), ptr(db_il), _ptr_array(dw_ih),
                                      _ptr_array(dw_hh), _ptr_array(db), _ptr_array(db2) if two_biases else None, stream()),
          "asr_lstm_unpack2_f32")
    return (dw_ih, dw_hh, db, db2) if two_biases else (dw_ih, dw_hh, db)


def lstm_pack_multi(layers, ndir):
    """layers: per layer the list of per-direction (w_ih, w_hh, b_ih, b_hh) in torch layout -> per layer (w_ih_cat
    [ndir*4H, I], w_hh_il [ndir, 4H, H], bias [ndir*4H]) in the kernels' gate-interleaved layout; one launch for up to
    PACK_MAX_LAYERS layers."""
    outs, keep = [], []
    jobs = (LstmPackJob * len(layers))()
    for j, params in enumerate(layers):
        H, I = params[1].shape[1], params[0].shape[1]
        ps = [p if p.is_contiguous() else p.contiguous() for p in params]
        keep.append(ps)
        f32 = dict(device=ps[0].device, dtype=torch.float32)
        out = (torch.empty(ndir * 4 * H, I, **f32), torch.empty(ndir, 4 * H, H, **f32), torch.empty(ndir * 4 * H, **f32))
        outs.append(out)
        job = jobs[j]
        job.H, job.I, job.ndir = H, I, ndir
        for d in range(ndir):
            job.w_ih[d], job.w_hh[d] = _dev(ps[4 * d]).data_ptr(), _dev(ps[4 * d + 1]).data_ptr()
            job.b_ih[d], job.b_hh[d] = _dev(ps[4 * d + 2]).data_ptr(), _dev(ps[4 * d + 3]).data_ptr()
        job.w_ih_cat, job.w_hh_il, job.bias = out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()
    lib = load()
    for j0 in range(0, len(layers), PACK_MAX_LAYERS):
        n = min(PACK_MAX_LAYERS, len(layers) - j0)
        check(lib.asr_lstm_pack_multi_f32(n, ctypes.cast(ctypes.byref(jobs, j0 * ctypes.sizeof(LstmPackJob)),
                                                         ctypes.POINTER(LstmPackJob)), stream()), "asr_lstm_pack_multi_f32")
    return outs


def lstm_unpack_multi(grads, dims, ndir):
    """grads: per layer (dw_ih_cat, dw_hh_il, db_il) in the interleaved layout (a layer whose three are all None gets no
    gradients), dims: per layer (H, I) -> per layer [per direction dw_ih, dw_hh, db_ih, db_hh] flattened in torch layout
    (b_ih and b_hh get their own tensors); one launch."""
    live = [j for j, g in enumerate(grads) if g[0] is not None]
    outs, keep = [None] * len(grads), []
    jobs = (LstmUnpackJob * max(len(live), 1))()
    for k, j in enumerate(live):
        H, I = dims[j]
        dw_ih, dw_hh, db = [g if g.is_contiguous() else g.contiguous() for g in grads[j]]
        keep.append((dw_ih, dw_hh, db))
        f32 = dict(device=dw_ih.device, dtype=torch.float32)
        o = []
        job = jobs[k]
        job.H, job.I, job.ndir = H, I, ndir
        job.dw_ih_cat, job.dw_hh_il, job.db_il = _dev(dw_ih).data_ptr(), _dev(dw_hh).data_ptr(), _dev(db).data_ptr()
        for d in range(ndir):
            t = [torch.empty(4 * H, I, **f32), torch.empty(4 * H, H, **f32), torch.empty(4 * H, **f32), torch.empty(4 * H, **f32)]
            job.dw_ih[d], job.dw_hh[d], job.db[d], job.db2[d] = [x.data_ptr() for x in t]
            o += t
        outs[j] = o
    lib = load()
    for k0 in range(0, len(live), PACK_MAX_LAYERS):
        n = min(PACK_MAX_LAYERS, len(live) - k0)
        check(lib.asr_lstm_unpack_multi_f32(n, ctypes.cast(ctypes.byref(jobs, k0 * ctypes.sizeof(LstmUnpackJob)),
                                                           ctypes.POINTER(LstmUnpackJob)), stream()), "asr_lstm_unpack_multi_f32")
    return outs


def dec_prepare(tokens, emb_w, xmask, X, Xd, fed, L, B, D, O, E):
    """Teacher-forced decoder input (embedding gather into X / Xd, zero recurrent slots, fed = tokens^T) in one launch.
    tokens [B, >= L] int64 on the device (row stride free)."""
    assert tokens.dtype == torch.long and tokens.is_cuda and tokens.stride(1) == 1 and tokens.shape[1] >= L
    assert X.is_contiguous() and (Xd is None or Xd.is_contiguous()) and fed.is_contiguous() and emb_w.is_contiguous()
    check(load().asr_dec_prepare_f32(L, B, D, O, E, c_p(tokens.data_ptr()), tokens.stride(0), ptr(emb_w),
                                     ptr(xmask) if xmask is not None else None, ptr(X), ptr(Xd) if Xd is not None else None,
                                     c_p(fed.data_ptr()), stream()), "asr_dec_prepare_f32")


def cell_pack(w_ih, w_hh, b_ih, b_hh, D, O, E, wcat, bcat):
    check(load().asr_cell_pack_f32(D, O, E, ptr(w_ih.contiguous()), ptr(w_hh.contiguous()), ptr(b_ih.contiguous()),
                                   ptr(b_hh.contiguous()), ptr(wcat), ptr(bcat), stream()), "asr_cell_pack_f32")


def dec_pack(w_ih, w_hh, b_ih, b_hh, wdec, watt, D, O, E, A, C, wcat, bcat, wcatT=None, wdecT=None, wattT=None):
    """cell_pack + the transposed images wcatT [KX, 4D], wdecT [D, A], wattT [C, A] (each optional) in one launch."""
    check(load().asr_dec_pack_f32(D, O, E, A, C, ptr(w_ih.contiguous()), ptr(w_hh.contiguous()), ptr(b_ih.contiguous()),
                                  ptr(b_hh.contiguous()), ptr(wdec.contiguous()), ptr(watt.contiguous()), ptr(wcat), ptr(bcat),
                                  ptr(wcatT), ptr(wdecT), ptr(wattT), stream()), "asr_dec_pack_f32")


def cell_unpack(dwcat, db_il, D, O, E):
    """-> dw_ih, dw_hh, db_ih, db_hh (the two bias gradients are equal, in tensors of their own)."""
    f32 = dict(device=dwcat.device, dtype=torch.float32)
    dw_ih, dw_hh, db, db2 = (torch.empty(4 * D, E + O, **f32), torch.empty(4 * D, D, **f32), torch.empty(4 * D, **f32),
                             torch.empty(4 * D, **f32))
    check(load().asr_cell_unpack_f32(D, O, E, ptr(dwcat), ptr(db_il), ptr(dw_ih), ptr(dw_hh), ptr(db), ptr(db2), stream()),
          "asr_cell_unpack_f32")
    return dw_ih, dw_hh, db, db2


_warned_embedding = []


def _embedding_layout_ok(tokens, grad, demb):
    V, E = demb.shape
    return not (grad.stride(1) != 1 or grad.shape != (tokens.numel(), E) or not tokens.is_contiguous() or not demb.is_contiguous()
                or E % 4 or grad.stride(0) % 4 or V * E * 4 > 65536 or E // 4 > 256 or grad.data_ptr() % 16)


def embedding_grad(tokens, grad, demb):
    """demb [V, E] += grad[r] for the token of row r (tokens [rows] int64, -1 = none; grad [rows, E] row-strided view).
    False when the layout is outside the kernel's (the caller then uses index_add_)."""
    V, E = demb.shape
    rows = tokens.numel()
    if DETERMINISTIC[0] and not _embedding_layout_ok(tokens, grad, demb) and not _warned_embedding:
        # the caller's own path is torch's index_add_, which adds with float atomics: say once that the mode ends here
        import warnings
        _warned_embedding.append(True)
        warnings.warn("deterministic mode: the embedding gradient [%d x %d] is outside asr_embedding_grad_det_f32's layout "
                      "(E %% 4, V * E * 4 <= 64 KB, 16-byte aligned rows); the caller's index_add_ is not run-to-run "
                      "reproducible" % (V, E), RuntimeWarning, stacklevel=2)
    if (grad.stride(1) != 1 or grad.shape != (rows, E) or not tokens.is_contiguous() or not demb.is_contiguous()
            or E % 4 or grad.stride(0) % 4 or V * E * 4 > 65536 or E // 4 > 256 or grad.data_ptr() % 16):
        return False
    entry = load().asr_embedding_grad_det_f32 if DETERMINISTIC[0] else load().asr_embedding_grad_f32
    check(entry(rows, E, V, c_p(tokens.data_ptr()), ptr(grad), grad.stride(0), ptr(demb), stream()),
          "asr_embedding_grad_det_f32" if DETERMINISTIC[0] else "asr_embedding_grad_f32")
    return True


def gather_sumsq(srcs, offsets, flat, sumsq=None):
    """flat[offsets[j] : + srcs[j].numel()] = srcs[j] (contiguous fp32 device tensors) in one launch; sumsq (1-element
    tensor or None) += the sum of their squares."""
    n = len(srcs)
    if DETERMINISTIC[0]:
        ws, nbytes = det_workspace(flat.device, 4 * sum((int(t.numel()) + 8191) // 8192 for t in srcs) if sumsq is not None else 0)
        check(load().asr_gather_sumsq_det_f32(n, _ptr_array(srcs), (c_i64 * n)(*[int(o) for o in offsets]),
                                              (c_i64 * n)(*[int(t.numel()) for t in srcs]), ptr(flat), ptr(sumsq), ws, nbytes,
                                              stream()), "asr_gather_sumsq_det_f32")
        return
    check(load().asr_gather_sumsq_f32(n, _ptr_array(srcs), (c_i64 * n)(*[int(o) for o in offsets]),
                                      (c_i64 * n)(*[int(t.numel()) for t in srcs]), ptr(flat), ptr(sumsq), stream()),
          "asr_gather_sumsq_f32")


SUMSQ_DET_WS_BYTES = 4096          # ASR_SUMSQ_DET_WS_BYTES


def sumsq(g, out):
    """out[0] += sum(g^2) over a flat fp32 device tensor (asr_sumsq_f32; asr_sumsq_det_f32 in deterministic mode)."""
    if DETERMINISTIC[0]:
        ws, nbytes = det_workspace(g.device, SUMSQ_DET_WS_BYTES)
        check(load().asr_sumsq_det_f32(g.numel(), ptr(g), ptr(out), ws, nbytes, stream()), "asr_sumsq_det_f32")
    else:
        check(load().asr_sumsq_f32(g.numel(), ptr(g), ptr(out), stream()), "asr_sumsq_f32")
    return out


def sum_det(x, out, scale=1.0):
    """out[0] += scale * sum(x) in a fixed order (asr_sum_det_f32): x a contiguous fp32 device tensor."""
    check(load().asr_sum_det_f32(x.numel(), ptr(x), float(scale), ptr(out), stream()), "asr_sum_det_f32")
    return out


def colsum_parts(parts):
    """parts: up to four [rows, ...] contiguous tensors with the same `rows` -> their sums over dim 0, one launch."""
    rows = parts[0].shape[0]
    outs = [torch.empty(p.shape[1:], device=p.device, dtype=torch.float32) for p in parts]
    n = (ctypes.c_int32 * len(parts))(*[int(p.numel() // rows) for p in parts])
    assert all(p.is_contiguous() and p.shape[0] == rows for p in parts) and len(parts) <= 4
    check(load().asr_colsum_parts_f32(len(parts), rows, _ptr_array(parts), n, _ptr_array(outs), stream()), "asr_colsum_parts_f32")
    return outs


def _off(t, elems):
    return c_p(_dev(t).data_ptr() + 4 * int(elems))


# the encoder on packed rows (RowLayout below; model.pBLSTM) - "padded": the time-major padded tensors (measurement)
USE_PACKED_ROWS = os.environ.get("ASR_ENCODER_ROWS", "packed") != "padded"
USE_PERSIST = os.environ.get("ASR_PERSIST", "1") != "0"
USE_PERSIST_DEC = USE_PERSIST and os.environ.get("ASR_PERSIST_DEC", "1") != "0"   # persistent decoder forward
USE_PERSIST_DEC_BWD = USE_PERSIST and os.environ.get("ASR_PERSIST_DEC_BWD", "1") != "0"   # ... and backward
# free-running decode: fused logits/argmax/next-embedding kernel per step (off: the same steps through torch glue)
USE_FEEDBACK_KERNEL = os.environ.get("ASR_FEEDBACK_KERNEL", "1") != "0"
# greedy decode without autograd: a group of 4 utterances stops once all of them have emitted <EOS> (what follows the
# first <EOS> is stripped by the CER path; the predictions of the skipped steps read <EOS>)
DECODE_EARLY_STOP = os.environ.get("ASR_DECODE_EARLY_STOP", "1") != "0"
_persist_scratch = {}
# exchange area of the persistent kernels: the largest user is the LSTM backward with exchanged dh partials,
# [8 groups][2 parities][32 dest][32 src][8 rows][H/32 units] floats = 8 MB at H = 512 (each launcher zeroes what it uses)
XCH_BYTES = 8 * 2 * 32 * 32 * 8 * 20 * 4      # the largest user: exchanged dh partials at H = 640 (20 units per CU), 10 MB
                                              # (= asr_persist_scratch_bytes(); persist_scratch checks it against the library)

# Which path every sequence operator actually took, per process: "<op>_persist" counts launches of the persistent
# XCD-local kernels, "<op>_step" counts sequences that ran on the per-step kernels instead (persistent path switched off,
# or the launcher answered ASR_E_SHAPE = -2: unsupported sizes / not an 8 x 32-CU device).  Ops: lstm_fwd, lstm_bwd,
# dec_fwd, dec_bwd, dec_free (free-running decode forward).  Tests assert on these so that a silent fallback cannot
# pass for the fast path; `with require_persistent():` turns a fallback into an error.
# "dec_bwd_det" counts decoder backward sequences of DETERMINISTIC mode (asr_dec_seq_bwd_det, or the per-step loop of the
# smooth feedback): the per-step kernels by the mode's choice, so neither a "dec_bwd_persist" nor a "dec_bwd_step" record is
# made and require_persistent() does not raise for them.
import collections
LAUNCHES = collections.Counter()
_REQUIRE_PERSIST = [os.environ.get("ASR_REQUIRE_PERSIST", "0") != "0"]


def count_path(op, persistent, why=""):
    LAUNCHES[op + ("_persist" if persistent else "_step")] += 1
    if not persistent and _REQUIRE_PERSIST[0]:
        raise RuntimeError("%s fell back to the per-step kernels (%s) while the persistent path was required" % (op, why))


ASR_E_SHAPE = -2             # include/asr_hip.h: a launcher's answer for sizes / a device its kernel does not cover


def persistent_ran(rc, what):
    """The return code of a persistent entry point -> True: it ran; False: it declined (ASR_E_SHAPE - the caller takes the
    per-step kernels); anything else is an error."""
    if rc == 0:
        return True
    if rc != ASR_E_SHAPE:
        check(rc, what)
    return False


def _scratch_ptrs(device):
    xch, ctrl = persist_scratch(device)
    return c_p(xch.data_ptr()), c_p(ctrl.data_ptr())


class require_persistent(object):
    """Context manager: any sequence operator that does not run on its persistent kernel raises."""

    def __enter__(self):
        self._old = _REQUIRE_PERSIST[0]
        _REQUIRE_PERSIST[0] = True
        return LAUNCHES

    def __exit__(self, *exc):
        _REQUIRE_PERSIST[0] = self._old
        return False


def _scratch_key(device):
    """One scratch pair per physical device: "cuda" and "cuda:0" name the same one."""
    d = torch.device(device)
    return "%s:%d" % (d.type, torch.cuda.current_device() if d.index is None else d.index) if d.type == "cuda" else str(d)


def persist_scratch(device, trace=False):
    """(xch, ctrl) scratch of the persistent kernels, one pair per device (calls are stream-ordered).  ctrl = 32 int32 words:
    [0] abort latch, [1] its code (set by any aborting launch, cleared only by persist_clear_abort), [16..31] the
    per-launch words the library zeroes before every launch (csrc/persist.h).  trace=True: a separate 4 KB control buffer
    whose words behind the per-launch block receive the clock stamps of the measurement builds (tools/)."""
    if trace:
        tkey = str(device) + "/trace"
        if tkey not in _persist_scratch:
            _persist_scratch[tkey] = (torch.zeros(XCH_BYTES // 8, dtype=torch.int64, device=device),
                                      torch.zeros(16384, dtype=torch.int32, device=device))     # 64 KB: tools/dec_trace2.py
        return _persist_scratch[tkey]
    key = _scratch_key(device)
    if key not in _persist_scratch:
        xb, cb = c_i64(0), c_i64(0)
        load().asr_persist_scratch_bytes(ctypes.byref(xb), ctypes.byref(cb))
        assert xb.value <= XCH_BYTES and cb.value <= 128, "libasr_hip.so wants a larger persistent scratch than this host code allocates"
        # one allocation: [128-byte control block | 10 MB exchange] so that the pre-launch reset is a single fill
        # (persist.h: persist_reset)
        base = torch.zeros(16 + XCH_BYTES // 8, dtype=torch.int64, device=device)
        _persist_scratch[key] = (base[16:], base[:16].view(torch.int32), base)
    return _persist_scratch[key][:2]


def persist_abort_code(device):
    """Which wait gave up first since the latch was cleared (ctrl[1]; 2 = unexpected workgroup placement, others = the
    poll site).  Synchronises."""
    key = _scratch_key(device)
    return int(_persist_scratch[key][1][1].item()) if key in _persist_scratch else 0


def persist_clear_abort(device):
    """Clear the abort latch (start of a step / after the caller has dealt with an abort); stream-ordered, no sync."""
    key = _scratch_key(device)
    if key in _persist_scratch:
        _persist_scratch[key][1][:2].zero_()


# An abort of the persistent kernels is a PLACEMENT problem - a workgroup that did not get its CU because another process's
# kernels held it, a bounded spin that expired behind one - and those pass.  So leaving the persistent kernels is a probation,
# not a verdict: after PERSIST_RETRY_STEPS train steps on the per-step kernels (3x slower at cfg-2) they are tried again,
# twice as late after every further abort (200, 400, ... capped at 64x).  0: never again (the behaviour up to round 4).
# Env ASR_PERSIST_RETRY_STEPS, config key `persist_retry_steps` (not a reference key).
PERSIST_RETRY_STEPS = int(os.environ.get("ASR_PERSIST_RETRY_STEPS", "200"))
_PROBATION = dict(wanted=None, aborts=0, steps=0, retry_at=None)


def disable_persistent(device=None, permanent=False):
    """Route every sequence operator of this process to the per-step HIP kernels (after an abort, or - permanent - when
    several processes share one GPU) and clear the abort latch.  Unless permanent, persistent_step_tick() brings the
    persistent kernels back after a probation (see PERSIST_RETRY_STEPS)."""
    global USE_PERSIST, USE_PERSIST_DEC, USE_PERSIST_DEC_BWD
    st = _PROBATION
    if st["wanted"] is None:
        st["wanted"] = (USE_PERSIST, USE_PERSIST_DEC, USE_PERSIST_DEC_BWD)       # what this process started with
    if permanent:
        st["wanted"] = (False, False, False)
    USE_PERSIST = USE_PERSIST_DEC = USE_PERSIST_DEC_BWD = False
    if not permanent:                 # (ranks sharing a card leave by decision, not after an abort: nothing to count, and a
        st["aborts"] += 1             #  later abort's probation starts at the base length)
    if permanent or PERSIST_RETRY_STEPS <= 0 or not any(st["wanted"]):
        st["retry_at"] = None
    else:
        st["retry_at"] = st["steps"] + PERSIST_RETRY_STEPS * (1 << min(st["aborts"] - 1, 6))
    if device is not None:
        persist_clear_abort(device)


def idle_xcd_mask(nbatch):
    """The XCDs NO persistent kernel of a step uses when a rank's batch has `nbatch` utterances (bit x = XCC id x), 0 when
    there are fewer than four.  Group g of a persistent launch is XCC id g; the LSTM kernels use ndir * ceil(nb / 4) groups
    for nb <= 16 rows (4-row groups, csrc/lstm_persist.hip: rows_per_group), the decoder kernels ceil(nb / 2) or ceil(nb / 4)
    (csrc/dec_persist.hip: DecGeo): eight utterances or fewer stay on XCDs 0-3.  Not with the per-step kernels (they use the
    whole chip) or with a forced row geometry (ASR_LSTM_ROWS: measurements)."""
    if not (USE_PERSIST and USE_PERSIST_DEC and USE_PERSIST_DEC_BWD) or os.environ.get("ASR_LSTM_ROWS"):
        return 0
    if _SIDE_FORCE_MASK is not None:           # measurement: ASR_SIDE_FORCE_MASK=0xff puts the products beside the chains of ANY batch
        return _SIDE_FORCE_MASK if int(nbatch) > 0 else 0
    return 0xF0 if 0 < int(nbatch) <= 8 else 0


_SIDE_FORCE_MASK = int(os.environ["ASR_SIDE_FORCE_MASK"], 0) & 0xff if os.environ.get("ASR_SIDE_FORCE_MASK") else None


def persistent_step_tick():
    """Called once per train step (Solver._step).  True when this call ended a probation: the sequence operators of the
    step that follows run on the persistent kernels again (an abort there is found and repeated like any other)."""
    global USE_PERSIST, USE_PERSIST_DEC, USE_PERSIST_DEC_BWD
    st = _PROBATION
    st["steps"] += 1
    if st["retry_at"] is None or st["steps"] < st["retry_at"]:
        return False
    USE_PERSIST, USE_PERSIST_DEC, USE_PERSIST_DEC_BWD = st["wanted"]
    st["retry_at"] = None
    return True


def persistent_probation():
    """(aborts so far, train steps until the persistent kernels are tried again or None)."""
    st = _PROBATION
    return st["aborts"], (None if st["retry_at"] is None else max(0, st["retry_at"] - st["steps"]))


def persist_aborted(device):
    """True if ANY persistent launch on `device` aborted since the latch was last cleared (synchronises; for tests /
    end-of-step checks).  The latch is sticky across launches: the per-launch abort word is zeroed before every launch,
    and a sequence operator is several launches."""
    key = _scratch_key(device)
    return key in _persist_scratch and int(_persist_scratch[key][1][0].item()) != 0


def persist_abort_flag(device):
    """The abort latch as a 1-element int32 device tensor (no sync): lets a data-parallel step add it to the values its
    all-reduce carries."""
    return persist_scratch(device)[1][:1]


class RowLayout(object):
    """Packed rows of the encoder (include/asr_hip.h, "PACKED ROWS"): per layer l = 0 .. n (n = the encoder output), batch
    row b owns ext[l][b] rows starting at base[l][b]; time t of utterance b sits at row base[l][b] + t.  The extents halve
    with the pyramid (ext[l] = 2 ext[l + 1] where layer l subsamples), so the pair-concat is a reshape of the row matrix,
    and every block ends with at least one padding row (ext > len).  Built on the host from the utterance lengths and
    uploaded once per batch (one non-blocking copy): `dev` [n + 1][3][B] int32 = (lens, base, ext) per layer."""

    ROW_QUANTUM = 16

    def __init__(self, ilens, subsample, device, t_pad=None):
        import numpy as np
        n = len(subsample)
        lens = [np.asarray([int(v) for v in ilens], dtype=np.int64)]
        pads = [int(max(ilens)) if t_pad is None else int(t_pad[0])]
        for i in range(n):
            lens.append((lens[-1] + 1) // 2 if subsample[i] > 1 else lens[-1].copy())
            pads.append(((pads[-1] + 1) // 2 if subsample[i] > 1 else pads[-1]) if t_pad is None else int(t_pad[i + 1]))
        ext = [None] * (n + 1)
        ext[n] = lens[n] + 1
        # The row counts are the M of the forward products and the K of the weight-gradient products.  The output's count is
        # rounded up to a multiple of ROW_QUANTUM = 16 (the extents double from there: 32 / 64 / 128 rows for a three-layer
        # pyramid), so that K % 32 == 0 where the GEMM's fast kernels want it and the layer-0 input projection has whole
        # 128-row tiles (its plain epilogue: 97 against 137 us at cfg-2).  The extra padding rows go to the shortest utterances
        # first (round robin); the recurrences run max(lens) steps whatever the extents are.
        odd = (-int(ext[n].sum())) % self.ROW_QUANTUM
        order = np.argsort(lens[n], kind="stable")
        while odd > 0:
            take = min(odd, len(ilens))
            ext[n][order[:take]] += 1
            odd -= take
        for i in range(n - 1, -1, -1):
            ext[i] = ext[i + 1] * 2 if subsample[i] > 1 else ext[i + 1].copy()
        self.B, self.n = len(ilens), n
        self.lens = [l.astype(np.int32) for l in lens]          # host copies (the launchers take rowext_host)
        self.ext = [np.ascontiguousarray(e.astype(np.int32)) for e in ext]
        self.base = [np.concatenate([[0], np.cumsum(e)[:-1]]).astype(np.int32) for e in ext]
        self.rows = [int(e.sum()) for e in ext]                 # R per layer
        self.steps = [int(l.max()) for l in lens]               # time steps the recurrence of layer l has to run (the kernels
                                                                # zero the padding rows of a block behind them themselves)
        self.t_pad = pads                                       # padded time extent per layer (the global one of a shard)
        table = np.stack([np.stack([self.lens[i], self.base[i], self.ext[i]]) for i in range(n + 1)])
        self.dev = to_device_i32(table, device)                 # [n + 1][3][B]

    def lens_dev(self, l):
        return self.dev[l, 0]

    def base_dev(self, l):
        return self.dev[l, 1]

    def ext_dev(self, l):
        return self.dev[l, 2]

    def replicated_rows(self, l):
        """Output rows of layer l's pair-concat whose second half is the reference's replicate-padded frame (model.py:85-88:
        an odd padded length T; only utterances of exactly that length see a non-zero replica): [(row of the pair)]."""
        import numpy as np
        T = self.t_pad[l]
        if T % 2 == 0:
            return []
        return [int((self.base[l][b] + T - 1) // 2) for b in np.nonzero(self.lens[l] == T)[0]]


class LayerRows(object):
    """One layer's view of a RowLayout: what the LSTM launchers need."""

    def __init__(self, layout, l):
        self.layout, self.l = layout, l
        self.B, self.R, self.T = layout.B, layout.rows[l], layout.steps[l]
        self.lens, self.base, self.ext = layout.lens_dev(l), layout.base_dev(l), layout.ext_dev(l)
        self.lens_host, self.ext_max = layout.lens[l], int(layout.ext[l].max())

    def host_ptr(self):
        return c_p(self.lens_host.ctypes.data)


def lstm_seq_fwd(gates, w_hh, lens, y, c, rows=None):
    """rows: a LayerRows - gates / y / c are then row matrices [R, 1, ...] in the packed layout (lens = rows.lens)."""
    T, B, ndir, H4 = gates.shape
    H = H4 // 4
    lib = load()
    rb, re, rh = (ptr(rows.base), ptr(rows.ext), rows.host_ptr()) if rows is not None else (None, None, None)
    if rows is not None:
        assert B == 1 and T == rows.R
        T, B = rows.T, rows.B
    if USE_PERSIST and persistent_ran(
            lib.asr_lstm_seq_fwd_persist(T, B, B, H, ndir, ptr(gates), ptr(w_hh), ptr(lens), rb, re, rh, ptr(y), ptr(c),
                                         *_scratch_ptrs(gates.device), ARITH[0], stream()), "asr_lstm_seq_fwd_persist"):
        count_path("lstm_fwd", True)
        return
    count_path("lstm_fwd", False, "H=%d B=%d ndir=%d persist=%s" % (H, B, ndir, USE_PERSIST))
    check(lib.asr_lstm_seq_fwd(T, B, B, H, ndir, ptr(gates), ptr(w_hh), ptr(lens), rb, re, ptr(y), ptr(c), stream()),
          "asr_lstm_seq_fwd")


def lstm_seq_bwd(gates, w_hhT, lens, dy, c, dcarry, y=None, dw_hh=None, db=None, w_hh=None, rows=None):
    """-> (fused_dw, fused_db): whether dW_hh and the bias gradient `db` were accumulated by the persistent kernel itself
    (db: by every persistent backward kernel; dW_hh: by all of them except the bf16x6 exchanged-partials kernel, see
    asr_lstm_bwd_persist_fuses_dw - the caller then forms it with a GEMM).
    w_hhT: the transposed recurrent weights [ndir][H][4H], or a callable producing them on demand; w_hh: the forward
    layout [ndir][4H][H] - when given, the kernel that can read it directly is tried first and the transpose is only
    formed if that kernel does not apply."""
    T, B, ndir, H4 = gates.shape
    H = H4 // 4
    lib = load()
    ar = ARITH[0]
    rb, re, rh = (ptr(rows.base), ptr(rows.ext), rows.host_ptr()) if rows is not None else (None, None, None)
    if rows is not None:                                   # packed rows (see lstm_seq_fwd): dW_hh is always the caller's
        assert B == 1 and T == rows.R
        T, B = rows.T, rows.B
    if DETERMINISTIC[0]:                                   # the fused dW_hh / db meet in atomics across the row groups: both are
        db = None                                          # the caller's (ordered) product and column sum instead
    fuses = (USE_PERSIST and rows is None and not DETERMINISTIC[0] and lib.asr_lstm_bwd_persist_fuses_dw(H, ar) == 1
             and y is not None and dw_hh is not None)
    yk, dwk = (y, dw_hh) if fuses else (None, None)
    def persistent(entry, what, w):
        return persistent_ran(entry(T, B, B, H, ndir, ptr(gates), ptr(w), ptr(lens), rb, re, rh, ptr(dy), ptr(c), ptr(yk),
                                    ptr(dwk), ptr(db), *_scratch_ptrs(gates.device), ar, stream()), what)

    if USE_PERSIST and w_hh is not None and persistent(lib.asr_lstm_seq_bwd_persist_w, "asr_lstm_seq_bwd_persist_w", w_hh):
        count_path("lstm_bwd", True)
        return fuses, db is not None
    if callable(w_hhT):
        w_hhT = w_hhT()
    if USE_PERSIST and persistent(lib.asr_lstm_seq_bwd_persist, "asr_lstm_seq_bwd_persist", w_hhT):
        count_path("lstm_bwd", True)
        return fuses, db is not None
    count_path("lstm_bwd", False, "H=%d B=%d ndir=%d persist=%s" % (H, B, ndir, USE_PERSIST))
    check(lib.asr_lstm_seq_bwd(T, B, B, H, ndir, ptr(gates), ptr(w_hhT), ptr(lens), rb, re, ptr(dy), ptr(c), ptr(dcarry),
                               stream()), "asr_lstm_seq_bwd")
    return False, False


# ---------------------------------------------------------------------------------------------------
# The decoder's sequence operators on a DecBuffers: as for the LSTM, the persistent kernel first, the per-step kernels when it is
# switched off or declines.
def dec_step_fwd(fs, s):
    """Decoder step s on the per-step kernels (fs: DecBuffers.fwd_struct())."""
    check(load().asr_dec_step_fwd(ctypes.byref(fs), s, stream()), "asr_dec_step_fwd")


def att_step_fwd(fs, s):
    """The attention half of step s alone: X[s + 1][:, :D] (the decoder state) and ws[s - 1] / w0 -> X[s + 1][:, D:D+O], ws[s]."""
    check(load().asr_att_step_fwd(ctypes.byref(fs), s, stream()), "asr_att_step_fwd")


def dec_step_bwd(bs, s):
    if DETERMINISTIC[0]:
        check(load().asr_dec_step_bwd_det(ctypes.byref(bs), s, stream()), "asr_dec_step_bwd_det")
        return
    check(load().asr_dec_step_bwd(ctypes.byref(bs), s, stream()), "asr_dec_step_bwd")


def dec_shape(buf):
    return "D=%(D)d A=%(A)d O=%(O)d E=%(E)d Tp=%(Tp)d B=%(B)d" % buf.dims


def dec_seq_fwd(buf):
    """All L steps over inputs that are complete in X / Xd before the first one (teacher forcing)."""
    lib, L = load(), buf.L
    fs = buf.fwd_struct()
    done = False
    if USE_PERSIST_DEC:          # one launch for the whole sequence
        entry = lib.asr_dec_seq_fwd_persist_fault if DEC_FAULT[0] else lib.asr_dec_seq_fwd_persist
        done = persistent_ran(entry(ctypes.byref(fs), *_scratch_ptrs(buf.X.device), stream()), "asr_dec_seq_fwd_persist")
    count_path("dec_fwd", done, dec_shape(buf))
    if not done:
        check(lib.asr_dec_seq_fwd(ctypes.byref(fs), 0, L, stream()), "asr_dec_seq_fwd")


def dec_free_fwd(buf, w_out, b_out, emb, logits, pred, fed, probs, tokens=None, tf_flags=None, smooth=False, smooth_scaling=1.0,
                 eos=-1):
    """Free-running steps: per step the decoder chain, then ONE kernel for logits + argmax + the next step's embedding input
    (teacher / predicted token, or the smooth embedding softmax(k*logit) @ E).  Step 0's input is in X[0] / Xd[0] already.
    w_out [V, D+O] (V <= 128), emb [V, E], tokens [B, L] long (scheduled sampling: tf_flags[s] picks teacher or prediction) -
    all contiguous; logits [L, B, V], pred / fed [L, B] long, probs [L-1, B, V] (smooth) are written.
    -> True when the persistent kernel ran the sequence."""
    B, L, DO, V = buf.B, buf.L, buf.dims["D"] + buf.dims["O"], w_out.shape[0]
    X, Xd, xmask, dev = buf.X, buf.Xd, buf.xmask, buf.X.device
    drop = Xd is not None
    fs = buf.fwd_struct()
    done = False
    if USE_PERSIST_DEC and (tokens is None or not smooth) and V <= 64:
        # the whole sequence in one launch, the feedback computed in the kernel: no teacher tokens at all, or
        # scheduled sampling (the host's per-step draws go along as a byte per step)
        # decoding without autograd: a group of 4 utterances stops once all of them have emitted <EOS>; the
        # outputs of the steps that are not run read <EOS> / zero logits / zero attention weights
        stop = DECODE_EARLY_STOP and eos >= 0 and not torch.is_grad_enabled() and tokens is None
        if stop:
            pred.fill_(eos)
            logits.zero_()
            buf.ws.zero_()
        tf_dev = None
        if tokens is not None:
            tf_dev = torch.tensor([1 if (tf_flags is None or tf_flags[i]) else 0 for i in range(L)],
                                  dtype=torch.uint8).to(dev, non_blocking=True)
        fb = DecFeedback(
            tokens=_lptr(tokens), ld_tokens=int(tokens.stride(0)) if tokens is not None else 0, teacher=_lptr(tf_dev),
            mode=2 if smooth else 1, V=V, eos=eos if stop else -1, scaling=float(smooth_scaling), w_out=_fptr(w_out),
            b_out=_fptr(b_out.contiguous()), emb=_fptr(emb), logits=_fptr(logits), probs=_fptr(probs) if smooth else None,
            pred=_lptr(pred), fed=_lptr(fed))
        done = persistent_ran(load().asr_dec_seq_fwd_persist_free(ctypes.byref(fs), ctypes.byref(fb), *_scratch_ptrs(dev),
                                                                  stream()), "asr_dec_seq_fwd_persist_free")
        if done and stop and L > 1:
            # the last step's logits come from X[L], which a stopped group never wrote: rows that had
            # already emitted <EOS> keep the pre-filled outputs
            lg_last = torch.empty(B, V, device=dev, dtype=torch.float32)
            pr_last = torch.empty(B, dtype=torch.long, device=dev)
            dec_feedback_fwd(X[L][:, :DO], w_out, b_out, emb, lg_last, pr_last, FEED_NONE)
            live = pred[:L - 1].ne(eos).all(0)
            pred[L - 1] = torch.where(live, pr_last, pred[L - 1])
            logits[L - 1] = torch.where(live.unsqueeze(1), lg_last, logits[L - 1])
        elif done:
            dec_feedback_fwd(X[L][:, :DO], w_out, b_out, emb, logits[L - 1], pred[L - 1], FEED_NONE)
    count_path("dec_free", done, "%s V=%d teacher=%s" % (dec_shape(buf), V, tokens is not None))
    if done:
        return True
    for s in range(L):
        dec_step_fwd(fs, s)
        last = s == L - 1
        if last:
            mode = FEED_NONE
        elif tokens is not None:
            mode = FEED_TEACHER if (tf_flags is None or tf_flags[s + 1]) else FEED_PREDICTED
        else:
            mode = FEED_SMOOTH if smooth else FEED_PREDICTED
        dec_feedback_fwd(
            X[s + 1][:, :DO], w_out, b_out, emb, logits[s], pred[s], mode, smooth_scaling,
            tok=tokens[:, s + 1] if mode == FEED_TEACHER else None, fed=None if last else fed[s + 1],
            probs=probs[s] if mode == FEED_SMOOTH else None,
            x_emb_next=None if last else X[s + 1][:, DO:],
            xd_emb_next=Xd[s + 1][:, DO:] if (drop and not last) else None,
            mask=xmask[s + 1][:, buf.dims["O"]:] if (drop and not last) else None)
    return False


def dec_seq_bwd(buf, acc, with_dws, persistent, teacher):
    """The backward of all L steps; the gradient of every step's [z, ctx] is in acc["G"][1:] already.  persistent: the forward's
    inputs were all tokens (teacher forcing, or scheduled sampling inside the persistent forward: no gradient flows through an
    argmax), so the persistent kernel may run it."""
    lib, L = load(), buf.L
    bs = buf.bwd_struct(acc=acc, with_dws=with_dws)
    done = False
    if DETERMINISTIC[0]:
        # the persistent backward adds its per-group partial sums of dgvec / dwatt / dconv with atomics: the per-step kernels
        # (one owner per partial sum), their two skinny products unsplit.  Not a fallback: the mode's choice, counted apart
        LAUNCHES["dec_bwd_det"] += 1
        check(lib.asr_dec_seq_bwd_det(ctypes.byref(bs), 0, L, stream()), "asr_dec_seq_bwd_det")
        return
    if USE_PERSIST_DEC_BWD and persistent:
        done = persistent_ran(lib.asr_dec_seq_bwd_persist(ctypes.byref(bs), _fptr(buf.Mf), *_scratch_ptrs(buf.X.device), stream()),
                              "asr_dec_seq_bwd_persist")
    count_path("dec_bwd", done, "%s teacher=%s" % (dec_shape(buf), teacher))
    if not done:
        check(lib.asr_dec_seq_bwd(ctypes.byref(bs), 0, L, stream()), "asr_dec_seq_bwd")


def dec_smooth_bwd(buf, acc, with_dws, w_out, emb, probs, scaling, dlog):
    """The backward of a free-running sequence with smooth-embedding feedback (model.py:341): emb_s = softmax(logit_{s-1}*k) @ E
    couples step s to the logits of step s-1.  probs [L-1, B, V]: the forward's softmax outputs; dlog [L*B, V]: the gradient
    of the logits from outside.  -> dtot [L, B, V] = dlog + what reaches the logits through the feedback (the weight gradients
    that depend on it are the caller's: one product each over the whole sequence)."""
    B, L, DO, V = buf.B, buf.L, buf.dims["D"] + buf.dims["O"], w_out.shape[0]
    bs = buf.bwd_struct(acc=acc, with_dws=with_dws)
    done = False
    if USE_PERSIST_DEC_BWD and L > 1 and not DETERMINISTIC[0]:
        # the whole free-running sequence in one launch: the feedback path (d(emb_s) -> logit_{s-1} -> [z, ctx]_{s-1})
        # is carried inside the persistent kernel (dec_persist.hip, template FB)
        dlfb = torch.zeros(L, B, V, device=dlog.device, dtype=torch.float32)
        fbs = DecFeedbackBwd(V=V, scaling=float(scaling), w_out=_fptr(w_out), emb=_fptr(emb), probs=_fptr(probs),
                             dlfb=_fptr(dlfb))
        done = persistent_ran(load().asr_dec_seq_bwd_persist_free(ctypes.byref(bs), ctypes.byref(fbs), _fptr(buf.Mf),
                                                                  *_scratch_ptrs(dlog.device), stream()),
                              "asr_dec_seq_bwd_persist_free")
    if DETERMINISTIC[0]:
        LAUNCHES["dec_bwd_det"] += 1
    else:
        count_path("dec_bwd", done, "free-running smooth: %s V=%d L=%d fused-feedback=True" % (dec_shape(buf), V, L))
    if done:
        return dlog.view(L, B, V) + dlfb
    # one kernel per step carries the embedding gradient back into logit_{s-1} and [z_{s-1}, c_{s-1}]
    G = acc["G"]
    dtot = dlog.clone().view(L, B, V)
    for s in range(L - 1, -1, -1):
        dec_step_bwd(bs, s)
        if s >= 1:
            dec_feedback_bwd(G[s][:, DO:], G[s][:, :DO], probs[s - 1], emb, w_out, scaling, dtot[s - 1])
    return dtot


# dropout masks regenerated inside the consuming kernels from a seed (off: materialised fp32 masks, as injected by tests)
USE_SEEDED_DROPOUT = os.environ.get("ASR_SEEDED_DROPOUT", "1") != "0"


class SeededMask(object):
    """Inverted-dropout mask given by (seed, p) over a tensor shape: mask(i) = keep(seed, i) / (1 - p) (dropout.hip)."""

    def __init__(self, shape, p, device, seed=None):
        self.shape, self.p, self.device = tuple(int(v) for v in shape), float(p), device
        # seeds come from torch's CPU generator: reproducible under torch.manual_seed, no device sync
        self.seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)

    def tensor(self):
        n = 1
        for v in self.shape:
            n *= v
        pad = torch.empty((n + 3) // 4 * 4, device=self.device, dtype=torch.float32)
        check(load().asr_dropout_mask_f32(pad.numel(), ptr(pad), self.seed, self.p, stream()), "asr_dropout_mask_f32")
        return pad[:n].view(self.shape)


def dropout_seeded_(x, m):
    """x *= mask in place (x contiguous, numel % 4 == 0)."""
    check(load().asr_dropout_seeded_f32(x.numel(), ptr(x), m.seed, m.p, stream()), "asr_dropout_seeded_f32")
    return x


def relu_dropout_bwd(grad, y, seed, p):
    """grad * mask * (y > 0) in one pass (p == 0: the plain relu gradient)."""
    out = torch.empty_like(y)
    check(load().asr_relu_dropout_bwd_f32(y.numel(), ptr(grad), ptr(y), int(seed), float(p), ptr(out), stream()),
          "asr_relu_dropout_bwd_f32")
    return out


def pyramid_fwd(x, mask, out):
    T, B, C = x.shape
    if isinstance(mask, SeededMask):
        check(load().asr_pyramid_concat_fwd_seeded(T, B, C, ptr(x), mask.seed, mask.p, ptr(out), stream()),
              "asr_pyramid_concat_fwd_seeded")
        return
    check(load().asr_pyramid_concat_fwd(T, B, C, ptr(x), ptr(mask), ptr(out), stream()), "asr_pyramid_concat_fwd")


def pyramid_bwd(dout, mask, din):
    T, B, C = din.shape
    if isinstance(mask, SeededMask):
        check(load().asr_pyramid_concat_bwd_seeded(T, B, C, ptr(dout), mask.seed, mask.p, ptr(din), stream()),
              "asr_pyramid_concat_bwd_seeded")
        return
    check(load().asr_pyramid_concat_bwd(T, B, C, ptr(dout), ptr(mask), ptr(din), stream()), "asr_pyramid_concat_bwd")


def rows_pack(x, rows):
    """x [B, T, C] (zero-padded batch, dataloader.py:6-12) -> [R, C] in the packed layout of `rows` (a LayerRows)."""
    B, T, C = x.shape
    out = torch.empty(rows.R, C, device=x.device, dtype=torch.float32)
    check(load().asr_rows_pack_f32(B, T, C, ptr(x), ptr(rows.lens), ptr(rows.base), ptr(rows.ext), rows.ext_max, ptr(out), stream()),
          "asr_rows_pack_f32")
    return out


def rows_unpack_fwd(packed, rows, T, fill, mask, fill_relu=False):
    """[R, C] -> [B, T, C]; frames behind an utterance = fill * mask (mask: None, a [B, T, C] tensor or a SeededMask);
    fill_relu: relu(fill) * mask (fill = the last projection's bias as it is)."""
    C = packed.shape[1]
    out = torch.empty(rows.B, T, C, device=packed.device, dtype=torch.float32)
    seeded = isinstance(mask, SeededMask)
    check(load().asr_rows_unpack_fwd_f32(rows.B, T, C, ptr(packed), ptr(rows.lens), ptr(rows.base), ptr(fill),
                                         1 if fill_relu else 0,
                                         None if (mask is None or seeded) else ptr(mask), mask.seed if seeded else 0,
                                         mask.p if seeded else 0.0, ptr(out), stream()), "asr_rows_unpack_fwd_f32")
    return out


def rows_unpack_bwd(dout, rows, C, mask, want_fill, relu_of=None, dfill=None):
    """-> (drows [R, C], dfill [C] or None).  relu_of: the fill vector in front of its relu (fill_relu of the forward): its
    gradient is masked by relu_of > 0.  dfill: a zeroed accumulator to use instead of a fresh one (the kernel adds to it).
    UnsupportedShape where the kernels refuse C: not a multiple of 4, or more than 512 float4 with the fill gradient."""
    B, T, _ = dout.shape
    drows = torch.empty(rows.R, C, device=dout.device, dtype=torch.float32)
    if not want_fill:
        dfill = None
    elif dfill is None:
        dfill = torch.zeros(C, device=dout.device, dtype=torch.float32)
    seeded = isinstance(mask, SeededMask)
    margs = (None if (mask is None or seeded) else ptr(mask), mask.seed if seeded else 0, mask.p if seeded else 0.0)
    det = DETERMINISTIC[0] and dfill is not None
    rc = load().asr_rows_unpack_bwd_f32(B, T, C, ptr(dout), ptr(rows.lens), ptr(rows.base), ptr(rows.ext), rows.ext_max,
                                        *margs, ptr(drows), None if det else ptr(dfill), ptr(relu_of), stream())
    if rc == ASR_E_SHAPE:                          # (refused before anything is launched: neither output is written)
        raise UnsupportedShape("rows_unpack_bwd: C %d (a multiple of 4; at most 2048 with the fill gradient)" % C)
    check(rc, "asr_rows_unpack_bwd_f32")
    if det:
        ws, nbytes = det_workspace(dout.device, B * C * 4)
        check(load().asr_rows_fill_grad_det_f32(B, T, C, ptr(dout), ptr(rows.lens), *margs, ptr(dfill), ptr(relu_of), ws, nbytes,
                                                stream()), "asr_rows_fill_grad_det_f32")
    return drows, dfill
