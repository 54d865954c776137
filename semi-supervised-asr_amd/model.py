"""MI355X-native seq2seq ASR model behind the reference's class surface.

Same class names, constructor signatures, forward signatures/returns and state_dict keys as
/root/reference/model.py (pBLSTM 58-98, Encoder 100-112, AttLoc 114-173, Decoder 256-367,
E2E 408-456, LM 459-573) — but every hot operator is a hand-written gfx950 kernel reached
through ops.py / hip_backend.py.  Activations are time-major inside the encoder, the decoder
loop is one fused graph node, and mlp_o is hoisted out of the step loop.
There is no CPU execution path: tensors must be on the GPU.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import hip_backend as hb
import ops
from hip_backend import to_device_i32 as hb_to_device
from utils import cc, pad_list, _seq_mask


class _LstmWeights(torch.nn.Module):
    """Parameter container with torch.nn.LSTM's names / shapes / default init (U(-1/sqrt(H), 1/sqrt(H)))
    so checkpoints interchange with the reference.  It has no forward of its own."""

    def __init__(self, input_dim, hidden_dim, num_layers=1, bidirectional=False):
        super().__init__()
        self.input_size, self.hidden_size = input_dim, hidden_dim
        self.num_layers, self.bidirectional = num_layers, bidirectional
        k = 1.0 / math.sqrt(hidden_dim)
        for layer in range(num_layers):
            idim = input_dim if layer == 0 else hidden_dim * (2 if bidirectional else 1)
            for suffix in ([""] + (["_reverse"] if bidirectional else [])):
                for name, shape in (("weight_ih", (4 * hidden_dim, idim)), ("weight_hh", (4 * hidden_dim, hidden_dim)),
                                    ("bias_ih", (4 * hidden_dim,)), ("bias_hh", (4 * hidden_dim,))):
                    p = torch.nn.Parameter(torch.empty(*shape).uniform_(-k, k))
                    self.register_parameter("%s_l%d%s" % (name, layer, suffix), p)

    def direction_params(self, layer):
        out = []
        for suffix in ([""] + (["_reverse"] if self.bidirectional else [])):
            out += [getattr(self, "%s_l%d%s" % (n, layer, suffix)) for n in
                    ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        return out


class _CellWeights(torch.nn.Module):
    """torch.nn.LSTMCell-shaped parameter container (weight_ih, weight_hh, bias_ih, bias_hh)."""

    def __init__(self, input_dim, hidden_dim):
        super().__init__()
        k = 1.0 / math.sqrt(hidden_dim)
        self.weight_ih = torch.nn.Parameter(torch.empty(4 * hidden_dim, input_dim).uniform_(-k, k))
        self.weight_hh = torch.nn.Parameter(torch.empty(4 * hidden_dim, hidden_dim).uniform_(-k, k))
        self.bias_ih = torch.nn.Parameter(torch.empty(4 * hidden_dim).uniform_(-k, k))
        self.bias_hh = torch.nn.Parameter(torch.empty(4 * hidden_dim).uniform_(-k, k))


def _drop_mask(shape, p, device):
    """Inverted-dropout mask, already scaled by 1/(1-p): on the GPU a (seed, p) descriptor that the consuming kernels
    expand in flight (hip_backend.SeededMask), otherwise / with ASR_SEEDED_DROPOUT=0 a materialised tensor.  Tests
    replace this function to inject given masks."""
    if hb.USE_SEEDED_DROPOUT and torch.device(device).type == "cuda":
        return hb.SeededMask(shape, p, device)
    return torch.empty(shape, device=device, dtype=torch.float32).bernoulli_(1.0 - p).mul_(1.0 / (1.0 - p))


def _mask_tensor(mask):
    return mask.tensor() if isinstance(mask, hb.SeededMask) else mask


def padded_lengths(t_max, n_layers, subsample):
    """Padded time extent entering each encoder layer (+ the output extent)."""
    out = [int(t_max)]
    for i in range(n_layers):
        out.append((out[-1] + 1) // 2 if subsample[i] > 1 else out[-1])
    return out


class pBLSTM(torch.nn.Module):
    """Pyramidal BiLSTM stack (model.py:58-98)."""

    def __init__(self, input_dim, hidden_dim, n_layers, subsample, dropout_rate):
        super(pBLSTM, self).__init__()
        layers, project_layers = [], []
        for i in range(n_layers):
            idim = input_dim if i == 0 else hidden_dim
            project_dim = hidden_dim * 4 if subsample[i] > 1 else hidden_dim * 2
            layers.append(_LstmWeights(idim, hidden_dim, num_layers=1, bidirectional=True))
            project_layers.append(torch.nn.Linear(project_dim, hidden_dim))
        self.layers = torch.nn.ModuleList(layers)
        self.project_layers = torch.nn.ModuleList(project_layers)
        self.dropout_layer = torch.nn.Dropout(p=dropout_rate)
        self.subsample = subsample
        self.dropout_rate = dropout_rate

    @property
    def time_reduction(self):
        """Input frames per output frame: 2 for every layer that subsamples (an utterance of n input frames leaves layer
        after layer with (n + 1) // 2), read from the layers this stack was built with."""
        r = 1
        for i in range(len(self.layers)):
            r *= 2 if self.subsample[i] > 1 else 1
        return r

    def forward(self, xpad, ilens, total_length=None):
        """xpad [B,T,idim] zero padded, ilens descending host ints -> ([B,T',H], list[int]).
        `total_length` (list from padded_lengths) keeps a data-parallel shard at the global padded
        extent; default = max(ilens) like pad_packed_sequence (model.py:81).

        Default: PACKED ROWS (hb.RowLayout; include/asr_hip.h) - what pack_padded_sequence gives the reference's LSTM
        (model.py:79-81), kept for the whole stack: every utterance is a block of consecutive rows (its frames + at least one
        zero row), every product of the encoder a GEMM over sum(len) rows instead of B * T_max, the pair-concat a reshape.
        The padded batch only exists at the two ends: the collated input is packed by one kernel, the output is unpacked into
        the [B, T', H] tensor the decoder reads, its frames behind an utterance filled with what the reference computes
        there, dropout(relu(bias)) of the last projection.  ASR_ENCODER_ROWS=padded: the time-major padded
        path (measurement)."""
        if hb.USE_PACKED_ROWS and xpad.is_cuda and xpad.shape[2] % 4 == 0:
            return self._forward_packed(xpad, ilens, total_length)
        return self._forward_padded(xpad, ilens, total_length)

    def _forward_packed(self, xpad, ilens, total_length):
        dev = xpad.device
        layout = hb.RowLayout([int(l) for l in ilens], [self.subsample[i] for i in range(len(self.layers))], dev,
                              t_pad=total_length)
        drop = self.training and self.dropout_rate > 0
        p = self.dropout_rate
        x = hb.rows_pack(xpad if xpad.is_contiguous() else xpad.contiguous(), hb.LayerRows(layout, 0))      # [R_0, idim]
        packs = ops.lstm_pack([layer.direction_params(0) for layer in self.layers], 2)   # kernel layout, all layers: one launch
        for i, (layer, proj) in enumerate(zip(self.layers, self.project_layers)):
            rows = hb.LayerRows(layout, i)
            y = ops.lstm_layer(x, None, None, 2, rows=rows, packed=packs[i])                     # [R_i, 2H]
            mask = _drop_mask((rows.R, 1, y.shape[1]), p, dev) if drop else None
            if self.subsample[i] > 1:
                rep = layout.replicated_rows(i)
                rep = hb.to_device_i64(rep, dev) if rep else None
                y = ops.pyramid_concat(y.view(rows.R, 1, -1), mask, rep).view(rows.R // 2, -1)  # [R_{i+1}, 4H]
            elif mask is not None:
                y = y * _mask_tensor(mask).view_as(y)
            if drop:
                m2 = _drop_mask((y.shape[0], 1, proj.weight.shape[0]), p, dev)
                if isinstance(m2, hb.SeededMask) and y.shape[0] * proj.weight.shape[0] % 4 == 0:
                    x = ops.linear(y, proj.weight, proj.bias, relu=True, drop=m2)      # relu -> dropout in the op
                else:
                    x = ops.linear(y, proj.weight, proj.bias, relu=True) * _mask_tensor(m2).view(y.shape[0], -1)
            else:
                x = ops.linear(y, proj.weight, proj.bias, relu=True)
        n = len(self.layers)
        t_out = layout.t_pad[n]
        pad_mask = _drop_mask((layout.B, t_out, x.shape[1]), p, dev) if drop else None
        # (frames behind an utterance: dropout(relu(bias)) of the last projection, SURVEY F2 - the relu is the kernel's)
        out = ops.rows_unpack(x, hb.LayerRows(layout, n), t_out, self.project_layers[-1].bias, pad_mask, fill_relu=True)
        self.last_lens_dev = layout.lens_dev(n)                    # device copy of the output lengths
        self.last_layout = layout                                  # (tests: where each utterance's rows were)
        return out, [int(l) for l in layout.lens[n]]

    def _forward_padded(self, xpad, ilens, total_length=None):
        dev = xpad.device
        lens = [int(l) for l in ilens]
        # lengths entering every layer are known on the host up front: one non-blocking upload for all layers
        per_layer = [lens]
        for i in range(len(self.layers)):
            sub = self.subsample[i]
            per_layer.append([(l + 1) // sub for l in per_layer[-1]] if sub > 1 else per_layer[-1])
        lens_all = hb_to_device(per_layer, dev)                    # [n_layers+1, B] int32
        x = xpad.transpose(0, 1)                                   # time-major
        drop = self.training and self.dropout_rate > 0
        packs = ops.lstm_pack([layer.direction_params(0) for layer in self.layers], 2)
        for i, (layer, proj) in enumerate(zip(self.layers, self.project_layers)):
            steps = max(lens) if total_length is None else int(total_length[i])
            if steps != x.shape[0]:                                 # (a no-op slice still records a SliceBackward:
                x = x[:steps]                                      #  a zero fill + a copy per layer in the backward)
            if not x.is_contiguous():
                x = x.contiguous()
            lens_dev = lens_all[i]
            y = ops.lstm_layer(x, lens_dev, None, 2, packed=packs[i])          # [T,B,2H]
            mask = _drop_mask(y.shape, self.dropout_rate, dev) if drop else None
            sub = self.subsample[i]
            if sub > 1:
                y = ops.pyramid_concat(y, mask)                    # [ceil(T/2),B,4H]
                lens = [(l + 1) // sub for l in lens]
            elif mask is not None:
                y = y * _mask_tensor(mask)
            if drop:
                m2 = _drop_mask((y.shape[0], y.shape[1], proj.weight.shape[0]), self.dropout_rate, dev)
                if isinstance(m2, hb.SeededMask) and m2.shape[0] * m2.shape[1] * m2.shape[2] % 4 == 0:
                    x = ops.linear(y, proj.weight, proj.bias, relu=True, drop=m2)      # relu -> dropout in the op
                else:
                    x = ops.linear(y, proj.weight, proj.bias, relu=True) * _mask_tensor(m2)
            else:
                x = ops.linear(y, proj.weight, proj.bias, relu=True)
        self.last_lens_dev = lens_all[-1]                          # device copy of the output lengths
        return x.transpose(0, 1).contiguous(), [int(l) for l in lens]


class Encoder(torch.nn.Module):
    """model.py:100-112 (pass-through to enc2; the VGG front end is dead code in the reference)."""

    def __init__(self, input_dim, hidden_dim, n_layers, subsample, dropout_rate, in_channel=1):
        super(Encoder, self).__init__()
        self.enc2 = pBLSTM(input_dim=input_dim, hidden_dim=hidden_dim, n_layers=n_layers, subsample=subsample,
                           dropout_rate=dropout_rate)

    def forward(self, x, ilens, total_length=None):
        return self.enc2(x, ilens, total_length)


class AttLoc(torch.nn.Module):
    """Location-aware attention parameters (model.py:114-137).  The per-step arithmetic of
    AttLoc.forward (139-173) runs inside the fused decoder sequence (ops.decoder_sequence); this
    module owns the weights under the reference's names."""

    def __init__(self, encoder_dim, decoder_dim, att_dim, conv_channels, conv_kernel_size, att_odim):
        super(AttLoc, self).__init__()
        self.mlp_enc = torch.nn.Linear(encoder_dim, att_dim)
        self.mlp_dec = torch.nn.Linear(decoder_dim, att_dim, bias=False)
        self.mlp_att = torch.nn.Linear(conv_channels, att_dim, bias=False)
        self.loc_conv = torch.nn.Conv2d(1, conv_channels, (1, 2 * conv_kernel_size + 1),
                                        padding=(0, conv_kernel_size), bias=False)
        self.gvec = torch.nn.Linear(att_dim, 1, bias=False)
        self.mlp_o = torch.nn.Linear(encoder_dim, att_odim)
        self.encoder_dim, self.decoder_dim = encoder_dim, decoder_dim
        self.att_dim, self.att_odim, self.conv_channels = att_dim, att_odim, conv_channels
        self.reset()

    def reset(self):
        self.enc_length = None
        self.enc_h = None
        self.pre_compute_enc_h = None

    @staticmethod
    def initial_weights(enc_len, frames, device):
        """model.py:151-153: uniform over each utterance's valid frames, 0 on the padding (no host stall in the
        middle of the step: pinned staging + non-blocking copy)."""
        if torch.device(device).type != "cuda":
            lens = torch.tensor([float(l) for l in enc_len]).unsqueeze(1)
            grid = torch.arange(frames, dtype=torch.float32).unsqueeze(0)
            return (grid < lens).to(torch.float32) / lens
        w0 = np.zeros((len(enc_len), int(frames)), dtype=np.float32)     # the lengths are host ints: build it there,
        for b, l in enumerate(enc_len):                                 # one non-blocking upload instead of 5 launches
            w0[b, :int(l)] = np.float32(1.0) / np.float32(int(l))
        return hb.to_device_f32(w0, device)

    def forward(self, enc_pad, enc_len, dec_z, att_prev, scaling=2.0):
        """Single attention step with the reference's signature (model.py:139-173): returns (mlp_o(context), w).
        Caches mlp_enc(enc_h) and enc_h W_o^T until reset(), like the reference caches pre_compute_enc_h.
        Forward only: training differentiates through the fused decoder sequence instead."""
        bsz, frames, _ = enc_pad.shape
        if self.pre_compute_enc_h is None:
            self.enc_h = enc_pad
            self.enc_length = frames
            with torch.no_grad():
                self.pre_compute_enc_h = ops.linear(enc_pad, self.mlp_enc.weight, self.mlp_enc.bias)
                self._q = ops.linear(enc_pad, self.mlp_o.weight, None)
        if dec_z is None:
            dec_z = enc_pad.new_zeros(bsz, self.decoder_dim)
        if att_prev is None:
            att_prev = AttLoc.initial_weights(enc_len, frames, enc_pad.device)
        return ops.attention_step(enc_pad, self.pre_compute_enc_h, self._q, self.mlp_dec.weight, self.loc_conv.weight,
                                  self.mlp_att.weight, self.gvec.weight, self.mlp_o.bias,
                                  dec_z.view(bsz, self.decoder_dim), att_prev, scaling)


class Decoder(torch.nn.Module):
    """model.py:256-367."""

    def __init__(self, output_dim, embedding_dim, hidden_dim, attention, att_odim, dropout_rate, bos, eos, pad,
                 ls_weight=0, labeldist=None):
        super(Decoder, self).__init__()
        self.bos, self.eos, self.pad = bos, eos, pad
        self.embedding = torch.nn.Embedding(output_dim, embedding_dim, padding_idx=pad)
        self.LSTMCell = _CellWeights(embedding_dim + att_odim, hidden_dim)
        self.output_layer = torch.nn.Linear(hidden_dim + att_odim, output_dim)
        self.dropout_layer = torch.nn.Dropout(p=dropout_rate)
        self.attention = attention
        self.hidden_dim, self.att_odim, self.dropout_rate = hidden_dim, att_odim, dropout_rate
        self._tok_const = {}
        self._dist_dev = {}
        self.ls_weight = ls_weight
        self.labeldist = labeldist
        if labeldist is not None:
            # plain attribute, not a buffer -> absent from state_dict
            self.vlabeldist = cc(torch.from_numpy(np.array(labeldist, dtype=np.float32)))

    def zero_state(self, enc_pad, dim=None):
        """model.py:276-280."""
        return enc_pad.new_zeros(enc_pad.size(0), dim if dim else self.hidden_dim)

    def forward_step(self, emb, dec_z, dec_c, c, w, enc_pad, enc_len):
        """One decoder step with the reference's signature (model.py:283-294): dropout(cat[emb, c]) -> LSTMCell ->
        attention -> output layer; returns (logit, dec_z, dec_c, c, w).  Thin, forward-only entry for callers that drive
        the loop themselves (inspection, custom search): the products run on the library's GEMM and attention-step
        kernels, the gate arithmetic on torch elementwise ops.  Training and Decoder.forward never come through here -
        they run all steps inside the fused sequence kernels (ops.decoder_sequence), which is what the fixtures pin; the
        tests hold this method to that path."""
        with torch.no_grad():
            cell = self.LSTMCell
            cell_inp = self.dropout_layer(torch.cat([emb, c], dim=-1)).contiguous()
            gates = hb.gemm(cell_inp, cell.weight_ih, trans_b=True, bias=cell.bias_ih)
            hb.gemm(dec_z.contiguous(), cell.weight_hh, trans_b=True, bias=cell.bias_hh, out=gates, accumulate=True)
            gi, gf, gg, go = gates.chunk(4, dim=1)
            dec_c = torch.sigmoid(gf) * dec_c + torch.sigmoid(gi) * torch.tanh(gg)
            dec_z = torch.sigmoid(go) * torch.tanh(dec_c)
            c, w = self.attention(enc_pad, enc_len, dec_z, w)
            logit = hb.gemm(torch.cat([dec_z, c], dim=-1).contiguous(), self.output_layer.weight, trans_b=True,
                            bias=self.output_layer.bias)
        return logit, dec_z, dec_c, c, w

    def _label_matrices(self, ys, olength=None):
        """ys_in = [BOS, y], ys_out = [y, EOS], both padded with EOS (model.py:301-306): ys_in as a [B, L] matrix, ys_out
        as [B, L] (a view) AND in the time-major [L, B] order the loss kernel indexes the logits with (third result).
        One concatenation + one gather on the device with indices built on the host from the (host-known) label
        lengths, instead of 2B concatenations and 2B row copies that leave the GPU idle behind the launch queue."""
        lens = [int(y.size(0)) for y in ys]
        bsz, n = len(ys), int(sum(lens))
        steps = max(lens) + 1
        if olength is not None and olength > steps:
            steps = int(olength)
        dev = ys[0].device
        key = (str(dev), str(ys[0].dtype))
        const = self._tok_const.get(key)
        if const is None:
            const = torch.tensor([self.bos, self.eos], dtype=ys[0].dtype, device=dev)
            self._tok_const[key] = const
        flat = torch.cat([y.reshape(-1) for y in ys] + [const])          # [n + 2]; n = BOS slot, n + 1 = EOS slot
        idx = np.full((2, bsz * steps), n + 1, dtype=np.int32)
        t_in, t_out = idx[0].reshape(bsz, steps), idx[1].reshape(steps, bsz)       # [B, L] and [L, B]
        off = 0
        for b, ln in enumerate(lens):
            t_in[b, 0] = n
            t_in[b, 1:1 + ln] = np.arange(off, off + ln)
            t_out[:ln, b] = np.arange(off, off + ln)
            off += ln
        if dev.type == "cuda":
            didx = hb.to_device_i64(idx, dev)
        else:
            didx = torch.from_numpy(idx).to(torch.long)
        both = flat[didx]
        out_lb = both[1].view(steps, bsz)
        return both[0].view(bsz, steps), out_lb.t(), out_lb

    def forward(self, enc_pad, enc_len, ys=None, tf_rate=1.0, max_dec_timesteps=500, sample=False, smooth=False,
                scaling=1.0, label_smoothing=True, olength=None, loss_norm=None):
        """-> (logits [B,L,V], ys_log_probs [B,L], prediction [B,L], ws [B,L,T']).
        `olength` (not in the reference) forces the number of teacher-forced steps so every
        data-parallel shard decodes the global olength.
        `loss_norm` (not in the reference): the number of utterances B the caller's loss -sum(ys_log_probs) / (B L)
        (solver.py:377) divides by - the kernel that forms ys_log_probs then leaves that loss in `ys_log_probs.fused_loss`
        (a device scalar with the graph behind it; parallel.local_loss returns it)."""
        dev = enc_pad.device
        bsz, frames, _ = enc_pad.shape
        att = self.attention
        att.reset()
        have_ys = ys is not None and len(ys) > 0
        opts = dict(scaling=2.0, smooth=bool(smooth), smooth_scaling=float(scaling), sample=bool(sample),
                    bos=self.bos, eos=self.eos)      # attention temperature is the AttLoc default
        if ys is not None:
            tok_in, tok_out, tok_out_lb = self._label_matrices(ys, olength)
            steps = tok_out.size(1)
            # one numpy draw per step, also at tf_rate=1 and for step 0 (model.py:328)
            draws = [np.random.random_sample() <= tf_rate for _ in range(steps)]
            draws[0] = True
            # every step teacher-forced: the argmax of the logits is only an output, and the loss kernel below reads them anyway
            opts.update(tokens=tok_in.to(dev), tf_flags=draws, skip_pred=have_ys and all(draws) and not sample)
        if not have_ys:
            steps = max_dec_timesteps
        opts["L"] = steps
        p = self.dropout_rate
        if self.training and p > 0:
            opts["xmask"] = _mask_tensor(_drop_mask((steps, bsz, self.att_odim + self.embedding.embedding_dim), p, dev))
        P = ops.linear(enc_pad, att.mlp_enc.weight, att.mlp_enc.bias)
        Q = ops.linear(enc_pad, att.mlp_o.weight, None)
        w0 = AttLoc.initial_weights(enc_len, frames, dev)
        cell = self.LSTMCell
        logits, ws, pred = ops.decoder_sequence(
            P, Q, self.embedding.weight, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh,
            att.mlp_dec.weight, att.loc_conv.weight, att.mlp_att.weight, att.gvec.weight, att.mlp_o.bias,
            self.output_layer.weight, self.output_layer.bias, w0, opts)
        ws = ws.transpose(0, 1)
        # log_softmax -> gather target (or own prediction) -> label smoothing (model.py:354-366), one kernel each way
        index_lb = tok_out_lb.to(dev) if have_ys else pred                       # [L, B] like the time-major logits
        smooth_on = label_smoothing and self.ls_weight > 0 and self.training
        if smooth_on:
            key = str(dev)
            if key not in self._dist_dev:
                self._dist_dev[key] = self.vlabeldist.to(dev).float().contiguous()
        scale = -1.0 / float(loss_norm * steps) if loss_norm else 1.0
        res = ops.label_logprob(logits, index_lb, self._dist_dev[str(dev)] if smooth_on else None,
                                self.ls_weight if smooth_on else 0.0, with_sum=True, sum_scale=scale, with_argmax=pred is None)
        ys_log_probs, total = res[0], res[1]
        if pred is None:
            pred = res[2]
        prediction = pred.transpose(0, 1)
        ys_log_probs = ys_log_probs.transpose(0, 1)
        # sum of all entries (times the loss's constant), from the same kernel (parallel.local_loss uses it)
        if loss_norm:
            ys_log_probs.fused_loss, ys_log_probs.fused_loss_scale = total, scale
        else:
            ys_log_probs.fused_sum = total
        return logits.transpose(0, 1), ys_log_probs, prediction, ws

    def recognize_beams(self, enc_pad, enc_len, max_dec_timesteps, topk, length_penalty=0.0, nbest=False, *, lm=None,
                        lm_weight=0.0, ctc_logits=None, ctc_lens=None, ctc_decode_weight=0.0, ngram=None, ngram_weight=0.0,
                        ngram_bonus=0.0, word_lm=None, word_lm_weight=0.0, word_bonus=0.0, lexicon_only=False):
        """Beam search with beam width topk (1..16) - model.py:369-406, which the reference left unfinished; the semantics
        are DESIGN 4.8's.  Eval arithmetic (no dropout, attention temperature 2.0), per utterance; hypotheses are ranked by
        score / len**length_penalty (score: the sum of the tokens' log-probabilities, <EOS> included).
        lm (an LM module) with lm_weight != 0: shallow fusion - every candidate token's score is
        log p_asr + lm_weight * log p_lm, the LM stepped on the device beside the decoder, eval arithmetic.
        ctc_logits [B, T', V] (raw logits of a CTC head on enc_pad, blank = <PAD> = 0) and ctc_lens (int32 [B] on the device:
        the valid frames) with ctc_decode_weight in (0, 1]: joint CTC-attention decoding - a token scores
        (1 - w) log p_asr + w (psi(g c) - psi(g)) with psi the CTC prefix score, computed on the device per step; it combines
        with the LM's term.  At 0 (or without the logits) the search is the one without it.
        ngram (an ngram.NgramLM) or word_lm (a word_lm.WordLM), one of them: the n-gram automaton, or the lexicon
        and the word-level LM, inside the search - a candidate ranks by (base + ngram_weight lm) + ngram_bonus len, with a word
        LM (base + word_lm_weight lm) + word_bonus n_words, base being its score without this LM; lexicon_only keeps only
        sequences of lexicon words (an utterance may then end without a hypothesis: a row of <EOS> at -inf).  Both combine with
        lm and with ctc_decode_weight.  self.last_beams then keeps the device record of the call: dict(tokens int32 [B, topk, L],
        lengths, scores, parts: dict(att, lm), n_words - with ngram the tokens without <EOS>); without them it is None.
        -> (prediction [B, L] int64, scores [B]): the best hypothesis, <EOS>-padded to L = max_dec_timesteps; with
        nbest=True all topk hypotheses, ranked: ([B, topk, L], [B, topk]).  topk = 1 is greedy decoding."""
        ctc_decode_weight = float(ctc_decode_weight)
        if not 0.0 <= ctc_decode_weight <= 1.0:
            raise ValueError("ctc_decode_weight must lie in [0, 1], got %r" % (ctc_decode_weight,))
        ctc_t = None
        if ctc_decode_weight > 0:
            if ctc_logits is None or ctc_lens is None:
                raise ValueError("ctc_decode_weight %g needs ctc_logits and ctc_lens" % ctc_decode_weight)
            if self.pad != 0:
                raise ValueError("the CTC prefix score takes <PAD> = 0 as its blank; pad is %d" % self.pad)
            host = [int(n) for n in enc_len] if isinstance(enc_len, (list, tuple)) else None
            ctc_t = dict(logits=ctc_logits, frame_lens=ctc_lens, lens_host=host)
        self.check_ngram(ngram)
        self.check_word_lm(word_lm, ngram)
        lm_t = None
        if lm is not None:
            V = self.output_layer.weight.shape[0]
            if lm.output_dim != V:
                raise ValueError("the LM predicts %d tokens, the decoder %d" % (lm.output_dim, V))
            if (lm.bos, lm.eos) != (self.bos, self.eos):
                raise ValueError("the LM's <BOS>/<EOS> (%d, %d) are not the decoder's (%d, %d)"
                                 % (lm.bos, lm.eos, self.bos, self.eos))
            lm_t = dict(emb=lm.embedding.weight, layers=[lm.LSTM.direction_params(l) for l in range(lm.n_layers)],
                        w_out=lm.output_layer.weight, b_out=lm.output_layer.bias)
        att = self.attention
        att.reset()
        with torch.no_grad():
            P = ops.linear(enc_pad, att.mlp_enc.weight, att.mlp_enc.bias)
            Q = ops.linear(enc_pad, att.mlp_o.weight, None)
            w0 = AttLoc.initial_weights(enc_len, enc_pad.shape[1], enc_pad.device)
            cell = self.LSTMCell
            out = ops.beam_search(
                P, Q, self.embedding.weight, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh,
                att.mlp_dec.weight, att.loc_conv.weight, att.mlp_att.weight, att.gvec.weight, att.mlp_o.bias,
                self.output_layer.weight, self.output_layer.bias, w0, int(topk), int(max_dec_timesteps), self.bos,
                self.eos, length_penalty=float(length_penalty), lm=lm_t, lm_weight=float(lm_weight), ctc=ctc_t,
                ctc_weight=ctc_decode_weight, ngram=ngram, ngram_weight=float(ngram_weight), ngram_bonus=float(ngram_bonus),
                word_lm=word_lm, word_lm_weight=float(word_lm_weight), word_bonus=float(word_bonus),
                lexicon_only=bool(lexicon_only))
            tokens, scores = out[0], out[1]
            self.last_beams = None
            if len(out) > 3:
                self.last_beams = dict(tokens=tokens, lengths=out[2], scores=scores, parts=dict(att=out[3], lm=out[4]),
                                       n_words=out[5])
            tokens = tokens.long()
        if nbest:
            return tokens, scores
        return tokens[:, 0], scores[:, 0]

    def score_hypotheses(self, enc_pad, enc_len, hyp, hyp_len):
        """The second pass of two-pass decoding: hyp int32 [B, K, T] (padded, as ops.ctc_beam returns them) and
        hyp_len int32 [B, K] (-1: an unused slot, scored as the empty hypothesis and masked by the caller), both on the device
        -> (att fp32 [B, K]: the sum of the decoder's log-probabilities of hypothesis k's tokens and its <EOS> given utterance
        b, tok_out int64 [B K, T + 1]: every hypothesis with its <EOS>, <EOS>-padded, mask bool [B K, T + 1]: its len + 1
        positions).  One teacher-forced pass of T + 1 steps over B K rows on the sequence kernels, every row attending to its
        utterance's frames; eval arithmetic (no dropout, no label smoothing) whatever the module's mode, no autograd, and no
        host read: the lengths stay on the device, the step count is the shape's."""
        bsz, K, T = hyp.shape
        rows, steps, dev = bsz * K, T + 1, enc_pad.device
        att = self.attention
        att.reset()
        with torch.no_grad():
            n = hyp_len.reshape(rows, 1).clamp(min=0).long()
            pos = torch.arange(steps, device=dev).unsqueeze(0)
            body = torch.cat([hyp.reshape(rows, T).long(), torch.full((rows, 1), self.eos, dtype=torch.long, device=dev)], dim=1)
            tok_out = torch.where(pos < n, body, torch.full_like(body, self.eos))             # [y, <EOS>, <EOS>, ...]
            tok_in = torch.cat([torch.full((rows, 1), self.bos, dtype=torch.long, device=dev), tok_out[:, :-1]], dim=1)
            mask = pos <= n
            enc_rep = enc_pad.repeat_interleave(K, dim=0)
            len_rep = [int(l) for l in enc_len for _ in range(K)]
            opts = dict(scaling=2.0, smooth=False, smooth_scaling=1.0, sample=False, bos=self.bos, eos=self.eos,
                        tokens=tok_in.contiguous(), tf_flags=[True] * steps, skip_pred=True, L=steps)
            P = ops.linear(enc_rep, att.mlp_enc.weight, att.mlp_enc.bias)
            Q = ops.linear(enc_rep, att.mlp_o.weight, None)
            w0 = AttLoc.initial_weights(len_rep, enc_rep.shape[1], dev)
            cell = self.LSTMCell
            logits, _, _ = ops.decoder_sequence(
                P, Q, self.embedding.weight, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh,
                att.mlp_dec.weight, att.loc_conv.weight, att.mlp_att.weight, att.gvec.weight, att.mlp_o.bias,
                self.output_layer.weight, self.output_layer.bias, w0, opts)
            logp = ops.label_logprob(logits, tok_out.t().contiguous())                        # [L, B K], time-major
            att_score = torch.where(mask, logp.t(), torch.zeros((), device=dev)).sum(dim=1).view(bsz, K)
        return att_score, tok_out, mask

    def score_hypotheses_grad(self, enc_pad, enc_len, hyp_tokens, hyp_len, scores=True):
        """score_hypotheses with the graph behind it - the scoring pass of MWER training: hyp_tokens int32 or
        int64 [B, K, T] and hyp_len int32 [B, K] (< 0: an unused slot) on the device -> (att [B, K] or None without `scores`,
        logits [T + 1, B K, V] time-major with the graph behind them, tok_out_lb int64 [T + 1, B K], npos int32 [B K]: len + 1,
        0 for an unused slot - the operands of ops.mwer_loss).  The same teacher-forced pass of T + 1 steps over B K rows;
        what differs: P and Q are formed ONCE over the B utterances and their rows replicated K times by expand + reshape, so
        the backward is an ordered sum over K and not an index-add; dropout follows the module's mode through xmask; no label
        smoothing (the sequence probability is the model's own); the attention temperature is the search's (2.0).  No host
        read."""
        bsz, K, T = hyp_tokens.shape
        rows, steps, dev = bsz * K, T + 1, enc_pad.device
        att = self.attention
        att.reset()
        with torch.no_grad():
            n = hyp_len.reshape(rows, 1).clamp(min=0).long()
            pos = torch.arange(steps, device=dev).unsqueeze(0)
            body = torch.cat([hyp_tokens.reshape(rows, T).long(),
                              torch.full((rows, 1), self.eos, dtype=torch.long, device=dev)], dim=1)
            tok_out = torch.where(pos < n, body, torch.full_like(body, self.eos))             # [y, <EOS>, <EOS>, ...]
            tok_in = torch.cat([torch.full((rows, 1), self.bos, dtype=torch.long, device=dev), tok_out[:, :-1]], dim=1)
            tok_out_lb = tok_out.t().contiguous()
            live = hyp_len.reshape(rows) >= 0
            npos = torch.where(live, hyp_len.reshape(rows).clamp(max=T) + 1, torch.zeros_like(hyp_len.reshape(rows))).int()
        opts = dict(scaling=2.0, smooth=False, smooth_scaling=1.0, sample=False, bos=self.bos, eos=self.eos,
                    tokens=tok_in.contiguous(), tf_flags=[True] * steps, skip_pred=True, L=steps)
        p = self.dropout_rate
        if self.training and p > 0:
            opts["xmask"] = _mask_tensor(_drop_mask((steps, rows, self.att_odim + self.embedding.embedding_dim), p, dev))
        P = ops.linear(enc_pad, att.mlp_enc.weight, att.mlp_enc.bias)
        Q = ops.linear(enc_pad, att.mlp_o.weight, None)
        frames = enc_pad.shape[1]
        P = P.unsqueeze(1).expand(bsz, K, frames, P.shape[2]).reshape(rows, frames, P.shape[2])
        Q = Q.unsqueeze(1).expand(bsz, K, frames, Q.shape[2]).reshape(rows, frames, Q.shape[2])
        w0 = AttLoc.initial_weights([int(l) for l in enc_len for _ in range(K)], frames, dev)
        cell = self.LSTMCell
        logits, _, _ = ops.decoder_sequence(
            P, Q, self.embedding.weight, cell.weight_ih, cell.weight_hh, cell.bias_ih, cell.bias_hh,
            att.mlp_dec.weight, att.loc_conv.weight, att.mlp_att.weight, att.gvec.weight, att.mlp_o.bias,
            self.output_layer.weight, self.output_layer.bias, w0, opts)
        att_score = None
        if scores:
            logp = ops.label_logprob(logits, tok_out_lb)                                      # [L, B K], time-major
            mask = (pos <= n).t()
            att_score = torch.where(mask, logp, torch.zeros((), device=dev)).sum(dim=0).view(bsz, K)
        return att_score, logits, tok_out_lb, npos

    def check_lm(self, lm):
        """ValueError unless lm (an LM module, or None) predicts the decoder's vocabulary with its <BOS> / <EOS>."""
        if lm is None:
            return
        V = self.output_layer.weight.shape[0]
        if lm.output_dim != V:
            raise ValueError("the LM predicts %d tokens, the decoder %d" % (lm.output_dim, V))
        if (lm.bos, lm.eos) != (self.bos, self.eos):
            raise ValueError("the LM's <BOS>/<EOS> (%d, %d) are not the decoder's (%d, %d)" % (lm.bos, lm.eos, self.bos, self.eos))

    def check_ngram(self, ngram):
        """ValueError unless ngram (an ngram.NgramLM, or None) is over the decoder's vocabulary with its <BOS> / <EOS>, and
        <PAD> = 0 is free to be the CTC blank."""
        if ngram is None:
            return
        V = self.output_layer.weight.shape[0]
        if ngram.V != V:
            raise ValueError("the n-gram LM predicts %d tokens, the decoder %d" % (ngram.V, V))
        if (ngram.bos, ngram.eos) != (self.bos, self.eos):
            raise ValueError("the n-gram LM's <BOS>/<EOS> (%d, %d) are not the decoder's (%d, %d)"
                             % (ngram.bos, ngram.eos, self.bos, self.eos))
        if self.pad != 0:
            raise ValueError("the n-gram LM keeps id 0 for the CTC blank; pad is %d" % self.pad)

    def check_word_lm(self, word_lm, ngram=None):
        """ValueError unless word_lm (a word_lm.WordLM, or None) spells in the decoder's vocabulary, its <BOS> / <EOS> (where it
        names them) are the decoder's, <PAD> = 0 is free to be the CTC blank, and no n-gram LM is given beside it."""
        if word_lm is None:
            return
        if ngram is not None:
            raise ValueError("ngram and word_lm are two LMs for one search: pass one of them")
        V = self.output_layer.weight.shape[0]
        if word_lm.V != V:
            raise ValueError("the word LM spells in %d tokens, the decoder predicts %d" % (word_lm.V, V))
        for name, mine, theirs in (("<BOS>", self.bos, word_lm.bos), ("<EOS>", self.eos, word_lm.eos)):
            if theirs is not None and theirs != mine:
                raise ValueError("the word LM's %s (%d) is not the decoder's (%d)" % (name, theirs, mine))
        if word_lm.space in (self.bos, self.eos, self.pad):
            raise ValueError("the word LM's <space> (%d) is the decoder's <BOS>, <EOS> or <PAD>" % word_lm.space)
        if self.pad != 0:
            raise ValueError("the word LM keeps id 0 for the CTC blank; pad is %d" % self.pad)

    def check_context(self, context, word_lm=None):
        """ValueError unless context (a context.ContextGraph or ContextBatch, or None) is over the decoder's vocabulary, <PAD>
        = 0 is free to be the CTC blank, and no word LM is given beside it."""
        if context is None:
            return
        if word_lm is not None:
            raise ValueError("a context beside the word LM is not built: pass context with ngram, or alone")
        V = self.output_layer.weight.shape[0]
        if context.V != V:
            raise ValueError("the context is over %d tokens, the decoder predicts %d" % (context.V, V))
        if self.pad != 0:
            raise ValueError("the context keeps id 0 for the CTC blank; pad is %d" % self.pad)

    def rescore_ctc_beams(self, enc_pad, enc_len, ctc_logits, ctc_lens, topk, ctc_weight=0.5, length_penalty=0.0, *, lm=None,
                          lm_weight=0.0, ngram=None, ngram_weight=0.0, ngram_bonus=0.0, word_lm=None, word_lm_weight=0.0,
                          word_bonus=0.0, lexicon_only=False, eos_term=True, context=None, ctx_weight=1.0):
        """Two-pass decoding behind the encoder (E2E.recognize_two_pass): ops.ctc_beam over ctc_logits [B, T', V]
        (raw logits of a CTC head on enc_pad, blank = <PAD> = 0; ctc_lens int32 [B] on the device), score_hypotheses over
        the B topk rows, with lm and lm_weight != 0 LM.forward over the same rows, then the combination
        ((1 - w) att + w ctc + lm_weight lm) / (len + 1)**length_penalty and the ranking, ties to the search's order.
        -> (tokens int64 [B, topk, T' + 1] ranked and <EOS>-padded, scores [B, topk] with -inf in unused slots, the parts:
        dict(hyp, hyp_len, ctc, att, lm, order)).  No host read.
        With ngram (an ngram.NgramLM) the first pass is the fused search - ops.ctc_beam with the LM inside,
        ranking by (ctc + ngram_weight lm_ngram) + ngram_bonus len, the end-of-sentence term on - and the combination is
        ((1 - w) att + w ctc + lm_weight lm + ngram_weight lm_ngram + ngram_bonus len) / (len + 1)**length_penalty, ctc
        the search's ctc_score and lm_ngram its lm_score; the parts then also hold ngram (lm_ngram) and rank (the search's
        score).
        With word_lm (a word_lm.WordLM) the first pass is the search with the lexicon and the word LM inside
        (lexicon_only and eos_term are the search's), and the combination is
        ((((1 - w) att + w ctc) + lm_weight lm) + word_lm_weight lm_word) + word_bonus n_words, then / (len + 1)**length_penalty:
        fp32, the two products and the two sums of the word term each rounded on their own, where the n-gram term stands;
        the parts then also hold word_lm (lm_word), n_words and rank.
        With context (a context.ContextGraph or ContextBatch) the first pass searches with the phrase lists
        inside, alone or beside ngram, and the combination gains + ctx_weight ctx_score (the search's bias of the hypothesis)
        behind the n-gram term, one product and one sum; the parts then also hold context (ctx_score) and rank."""
        K, w = int(topk), float(ctc_weight)
        if self.pad != 0:
            raise ValueError("the CTC search takes <PAD> = 0 as its blank; pad is %d" % self.pad)
        self.check_lm(lm)
        self.check_ngram(ngram)
        self.check_context(context, word_lm)
        self.check_word_lm(word_lm, ngram)
        use_lm = lm is not None and float(lm_weight) != 0.0
        with torch.no_grad():
            ng = rank = n_words = cx = None
            if context is not None:
                beams = ops.ctc_beam(ctc_logits, ctc_lens, K, ngram=ngram, ngram_weight=ngram_weight, ngram_bonus=ngram_bonus,
                                     eos_term=True, context=context, ctx_weight=ctx_weight)
                hyp, hyp_len, rank, ctc = beams[:4]
                ng, cx = (beams[4] if ngram is not None else None), beams[-1]
            elif word_lm is not None:
                hyp, hyp_len, rank, ctc, ng, n_words = ops.ctc_beam(ctc_logits, ctc_lens, K, word_lm=word_lm,
                                                                    word_lm_weight=word_lm_weight, word_bonus=word_bonus,
                                                                    lexicon_only=lexicon_only, eos_term=eos_term)
            elif ngram is None:
                hyp, hyp_len, ctc = ops.ctc_beam(ctc_logits, ctc_lens, K)
            else:
                hyp, hyp_len, rank, ctc, ng = ops.ctc_beam(ctc_logits, ctc_lens, K, ngram=ngram, ngram_weight=ngram_weight,
                                                           ngram_bonus=ngram_bonus, eos_term=True)
            bsz, _, T = hyp.shape
            att, tok_out, mask = self.score_hypotheses(enc_pad, enc_len, hyp, hyp_len)
            lm_score = None
            if use_lm:
                was_training = lm.training
                lm.eval()
                try:
                    lm_logp, _, _ = lm(tok_out, discrete_input=False)
                finally:
                    lm.train(was_training)
                lm_score = torch.where(mask, lm_logp, torch.zeros((), device=lm_logp.device)).sum(dim=1).view(bsz, K)
            # (1 - w) att + w ctc + lm_weight lm: one rounding per operation (torch's elementwise kernels do not contract)
            w_t = torch.tensor(w, dtype=torch.float32)
            total = att * float(1.0 - w_t) + ctc * float(w_t)
            if use_lm:
                total = total + lm_score * float(torch.tensor(float(lm_weight), dtype=torch.float32))
            if ngram is not None:
                total = total + ng * float(torch.tensor(float(ngram_weight), dtype=torch.float32))
                total = total + hyp_len.clamp(min=0).to(torch.float32) * float(torch.tensor(float(ngram_bonus), dtype=torch.float32))
            if word_lm is not None:
                total = total + ng * float(torch.tensor(float(word_lm_weight), dtype=torch.float32))
                total = total + n_words.clamp(min=0).to(torch.float32) * float(torch.tensor(float(word_bonus), dtype=torch.float32))
            if context is not None:
                total = total + cx * float(torch.tensor(float(ctx_weight), dtype=torch.float32))
            if float(length_penalty) != 0.0:
                total = total / (hyp_len.clamp(min=0) + 1).to(torch.float32).pow(float(length_penalty))
            total = torch.where(hyp_len >= 0, total, torch.full_like(total, float("-inf")))
            order = torch.sort(total, dim=1, descending=True, stable=True).indices                # ties to the lower k
            scores = torch.gather(total, 1, order)
            tokens = torch.gather(tok_out.view(bsz, K, T + 1), 1, order.unsqueeze(2).expand(bsz, K, T + 1))
        parts = dict(hyp=hyp, hyp_len=hyp_len, ctc=ctc, att=att, lm=lm_score, order=order)
        if ngram is not None:
            parts.update(ngram=ng, rank=rank)
        if word_lm is not None:
            parts.update(word_lm=ng, n_words=n_words, rank=rank)
        if context is not None:
            parts.update(context=cx, rank=rank)
        return tokens, scores, parts


class TransducerHead(torch.nn.Module):
    """The transducer (RNN-T) head on the encoder output (not in the reference): a prediction network - an
    embedding and a one-layer unidirectional LSTM over <BOS>, y_1 .. y_U on ops.lstm_layer - and a joint network
    logits(t, u) = lin_out(tanh(lin_enc(enc_h[t]) + lin_pred(pred_h[u]))) whose products run on ops.linear and whose
    activations and loss are csrc/rnnt.hip's.  Blank = <PAD> = 0, never a label."""

    def __init__(self, output_dim, embedding_dim, pred_dim, enc_hidden_dim, joint_dim, bos):
        super(TransducerHead, self).__init__()
        if joint_dim <= 0 or joint_dim % 4:
            raise ValueError("rnnt_joint_dim must be a positive multiple of 4, got %r" % (joint_dim,))
        self.bos, self.pred_dim, self.joint_dim, self.output_dim = bos, pred_dim, joint_dim, output_dim
        self.embedding = torch.nn.Embedding(output_dim, embedding_dim)
        self.lstm = _LstmWeights(embedding_dim, pred_dim, num_layers=1, bidirectional=False)
        self.lin_enc = torch.nn.Linear(enc_hidden_dim, joint_dim)
        self.lin_pred = torch.nn.Linear(pred_dim, joint_dim, bias=False)
        self.lin_out = torch.nn.Linear(joint_dim, output_dim)

    def project_enc(self, enc_h):
        """enc_h [B, T', H] -> PE [B, T', J]."""
        bsz, frames, hid = enc_h.shape
        return ops.linear(enc_h.reshape(bsz * frames, hid), self.lin_enc.weight, self.lin_enc.bias).view(bsz, frames, -1)

    def predict(self, ys):
        """The prediction network over <BOS>, y_1 .. y_U of every utterance -> PP [B, U + 1, J] (U the longest transcript).
        Every row runs all U + 1 steps on zero-padded tokens: the network is causal, so the positions u <= U_b do not see the
        padding, and the positions behind them are padding nodes of the lattice, which nothing reads."""
        dev = self.embedding.weight.device
        bos = ys[0].new_tensor([self.bos])
        tok = pad_list([torch.cat([bos, y.reshape(-1)]) for y in ys], 0).to(device=dev, dtype=torch.long)
        bsz, steps = tok.shape
        x_tm = self.embedding(tok).transpose(0, 1).contiguous()
        h = ops.lstm_layer(x_tm, hb_to_device([steps] * bsz, dev), self.lstm.direction_params(0), 1)      # [U + 1, B, P]
        h = h.transpose(0, 1).contiguous()
        return ops.linear(h.view(bsz * steps, -1), self.lin_pred.weight).view(bsz, steps, -1)

    def logits(self, enc_h, ys, frame_lens_dev):
        """-> raw logits [B, T', U + 1, V] (zeros' image lin_out.bias on padding nodes, which the loss never reads)."""
        counts = [int(y.numel()) for y in ys]
        z = ops.rnnt_joint(self.project_enc(enc_h), self.predict(ys), frame_lens_dev, counts)
        bsz, frames, u1, jdim = z.shape
        return ops.linear(z.view(bsz * frames * u1, jdim), self.lin_out.weight, self.lin_out.bias).view(bsz, frames, u1, -1)

    def nll(self, enc_h, ys, frame_lens_dev):
        """Per-utterance transducer negative log-likelihood [B]."""
        logits = self.logits(enc_h, ys, frame_lens_dev)
        labels = torch.cat([y.reshape(-1) for y in ys]).to(device=enc_h.device, dtype=torch.long)
        return ops.rnnt_loss(logits, frame_lens_dev, labels, [int(y.numel()) for y in ys])

    def cell_step(self, tok, h, c):
        """One prediction-network step for all rows (decoding; no autograd): tok int [B], h / c [B, P] -> (h', c').  The
        products run on asr_gemm_f32, as LM.forward_step's do."""
        w_ih, w_hh, b_ih, b_hh = self.lstm.direction_params(0)
        x = self.embedding(tok.long()).contiguous()
        gates = hb.gemm(x, w_ih, trans_b=True, bias=b_ih)
        hb.gemm(h.contiguous(), w_hh, trans_b=True, bias=b_hh, out=gates, accumulate=True)
        gi, gf, gg, go = gates.chunk(4, dim=1)
        c2 = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
        return torch.sigmoid(go) * torch.tanh(c2), c2

    def greedy(self, enc_h, frame_lens_dev, max_symbols, max_len):
        """Greedy transducer decoding of enc_h [B, T', H]: lin_enc once, then a fixed T' + max_len iterations of (the greedy
        step kernel, one prediction-network cell step for all rows with h, c and the projection committed only where the
        kernel set `advance`).  No host read.  -> (tokens int32 [B, max_len], lengths int32 [B], scores fp32 [B]) on the
        device; a row emits at most max_symbols tokens per frame and max_len in all."""
        bsz, frames, _ = enc_h.shape
        dev = enc_h.device
        pe = self.project_enc(enc_h).contiguous()
        i32 = dict(device=dev, dtype=torch.int32)
        t_cur, n_out, n_frame, advance = (torch.zeros(bsz, **i32) for _ in range(4))
        last = torch.full((bsz,), self.bos, **i32)
        out = torch.zeros(bsz, max_len, **i32)
        score = torch.zeros(bsz, device=dev, dtype=torch.float32)
        zero = torch.zeros(bsz, self.pred_dim, device=dev, dtype=torch.float32)
        h, c = self.cell_step(last, zero, zero)
        w_out, b_out = self.lin_out.weight.contiguous(), self.lin_out.bias
        pp = hb.gemm(h.contiguous(), self.lin_pred.weight, trans_b=True)
        for _ in range(frames + max_len):
            hb.rnnt_greedy_step(pe, pp, w_out, b_out, frame_lens_dev, t_cur, n_out, n_frame, out, last, score, advance,
                                max_symbols)
            h2, c2 = self.cell_step(last, h, c)
            adv = advance.bool().unsqueeze(1)
            h, c = torch.where(adv, h2, h), torch.where(adv, c2, c)
            pp = hb.gemm(h.contiguous(), self.lin_pred.weight, trans_b=True)
        return out, n_out, score

    def beam(self, enc_h, frame_lens_dev, beam, max_len, ngram=None, ngram_weight=0.0, ngram_bonus=0.0, eos_term=True, *,
             word_lm=None, word_lm_weight=0.0, word_bonus=0.0, lexicon_only=False):
        """Beam search over the head on enc_h [B, T', H]: lin_enc once, the prediction cell's weights
        concatenated once ([w_ih | w_hh], b_ih + b_hh), then ops.rnnt_beam - a fixed T' + max_len iterations, no host read.
        -> (hyp int32 [B, beam, max_len] padded with -1, hyp_len int32 [B, beam], score fp32 [B, beam] descending) and, with
        ngram, (rnnt_score, lm_score) behind them: the conventions of ops.ctc_beam.  With word_lm (a word_lm.WordLM; DESIGN
        4.30) the lexicon and the word LM sit inside the search: (rnnt_score, lm_score, n_words) behind the three."""
        w_ih, w_hh, b_ih, b_hh = self.lstm.direction_params(0)
        w_gate = torch.cat([w_ih.detach(), w_hh.detach()], dim=1).contiguous()
        b_gate = (b_ih.detach() + b_hh.detach()).contiguous()
        return ops.rnnt_beam(self.project_enc(enc_h), frame_lens_dev, w_gate, b_gate, self.lin_pred.weight, self.lin_out.weight,
                             self.lin_out.bias, self.embedding.weight, self.bos, beam, max_len, ngram=ngram,
                             ngram_weight=ngram_weight, ngram_bonus=ngram_bonus, eos_term=eos_term, word_lm=word_lm,
                             word_lm_weight=word_lm_weight, word_bonus=word_bonus, lexicon_only=lexicon_only)


class E2E(torch.nn.Module):
    """model.py:408-456."""

    def __init__(self, input_dim, enc_hidden_dim, enc_n_layers, subsample, dropout_rate, dec_hidden_dim, att_dim,
                 conv_channels, conv_kernel_size, att_odim, embedding_dim, output_dim, ls_weight, labeldist,
                 pad=0, bos=1, eos=2, ctc_weight=0.0, rnnt_weight=0.0, rnnt_joint_dim=256, rnnt_pred_dim=None,
                 ctc_star_penalty=None):
        super(E2E, self).__init__()
        self.encoder = Encoder(input_dim=input_dim, hidden_dim=enc_hidden_dim, n_layers=enc_n_layers,
                               subsample=subsample, dropout_rate=dropout_rate)
        # one AttLoc shared as self.attention and decoder.attention (duplicate state_dict keys)
        self.attention = AttLoc(encoder_dim=enc_hidden_dim, decoder_dim=dec_hidden_dim, att_dim=att_dim,
                                conv_channels=conv_channels, conv_kernel_size=conv_kernel_size, att_odim=att_odim)
        self.decoder = Decoder(output_dim=output_dim, hidden_dim=dec_hidden_dim, embedding_dim=embedding_dim,
                               attention=self.attention, dropout_rate=dropout_rate, att_odim=att_odim,
                               ls_weight=ls_weight, labeldist=labeldist, bos=bos, eos=eos, pad=pad)
        # `ctc_weight` (not in the reference): w > 0 adds a CTC branch on the encoder output and trains on
        # (1 - w) L_att + w L_ctc.  The head exists only then: at 0 the parameters, the state_dict keys and
        # every launch are the reference model's.  Blank = <PAD> = index 0, which is never a label.
        self.ctc_weight = float(ctc_weight)
        if not 0.0 <= self.ctc_weight <= 1.0:
            raise ValueError("ctc_weight must lie in [0, 1], got %r" % (ctc_weight,))
        if self.ctc_weight > 0:
            if pad != 0:
                raise ValueError("the CTC branch takes <PAD> = 0 as its blank; pad is %d" % pad)
            self.ctc_lo = torch.nn.Linear(enc_hidden_dim, output_dim)
        # `ctc_star_penalty` (not in the reference): a float <= 0 makes the CTC term of a TRAINING step the star
        # CTC loss (ops.ctc_star_loss) - transcripts with missing words; None: the plain loss, launch for launch.  A plain
        # attribute, no parameter and no state_dict key: it may be reassigned between steps (a penalty schedule is the
        # caller's host arithmetic).  In eval mode the plain CTC loss runs, so a dev loss stays comparable.
        self.ctc_star_penalty = None if ctc_star_penalty is None else float(ctc_star_penalty)
        if self.ctc_star_penalty is not None:
            if self.ctc_weight <= 0:
                raise ValueError("ctc_star_penalty needs the CTC branch: ctc_weight is 0")
            if not self.ctc_star_penalty <= 0:
                raise ValueError("ctc_star_penalty must be <= 0, got %r" % (ctc_star_penalty,))
        # `rnnt_weight` (not in the reference): w > 0 adds the transducer head and trains on
        # (1 - w_ctc - w_rnnt) L_att + w_ctc L_ctc + w_rnnt L_rnnt.  Like the CTC branch the head exists only
        # then: at 0 its parameters, its state_dict keys and every launch are absent.
        self.rnnt_weight = float(rnnt_weight)
        if not 0.0 <= self.rnnt_weight <= 1.0:
            raise ValueError("rnnt_weight must lie in [0, 1], got %r" % (rnnt_weight,))
        if self.ctc_weight + self.rnnt_weight > 1.0:
            raise ValueError("ctc_weight + rnnt_weight must be at most 1, got %r + %r" % (ctc_weight, rnnt_weight))
        if self.rnnt_weight > 0:
            if pad != 0:
                raise ValueError("the transducer head takes <PAD> = 0 as its blank; pad is %d" % pad)
            self.rnnt = TransducerHead(output_dim=output_dim, embedding_dim=embedding_dim,
                                       pred_dim=int(rnnt_pred_dim) if rnnt_pred_dim else dec_hidden_dim,
                                       enc_hidden_dim=enc_hidden_dim, joint_dim=int(rnnt_joint_dim), bos=bos)

    accepts_loss_norm = True          # (parallel.sup_local_loss: this forward takes the loss's normaliser along)

    def forward(self, data, ilens, ys=None, tf_rate=1.0, max_dec_timesteps=200, sample=False, smooth=False,
                scaling=1.0, label_smoothing=True, total_length=None, olength=None, loss_norm=None):
        if data.is_cuda:
            hb.upload_side_stream_for(data.shape[0] * data.shape[1])       # small uploads leave the compute stream when the GPU is the bottleneck
        enc_h, enc_lens = self.encoder(data, ilens, total_length)
        out = self.decoder(enc_h, enc_lens, ys, tf_rate=tf_rate, max_dec_timesteps=max_dec_timesteps, sample=sample,
                           smooth=smooth, scaling=scaling, label_smoothing=label_smoothing, olength=olength,
                           loss_norm=loss_norm)
        if self.ctc_weight > 0 and ys is not None and len(ys) > 0:
            # the CTC term rides on ys_log_probs, where the attention loss's kernel sum rides already (Decoder.forward):
            # parallel.local_loss forms (1 - w) L_att + w L_ctc from them.  Decoding (ys=None) never gets here.
            nll = self.ctc_nll(enc_h, ys)
            norm = float(loss_norm) if loss_norm else float(len(ys))
            lp = out[1]
            lp.ctc_nll, lp.ctc_loss, lp.ctc_norm, lp.ctc_weight = nll, nll.sum() * (1.0 / norm), norm, self.ctc_weight
        if self.rnnt_weight > 0 and ys is not None and len(ys) > 0:
            # the transducer term rides the same way (parallel.joint_loss)
            nll = self.rnnt_nll(enc_h, ys)
            norm = float(loss_norm) if loss_norm else float(len(ys))
            lp = out[1]
            lp.rnnt_nll, lp.rnnt_loss, lp.rnnt_norm, lp.rnnt_weight = nll, nll.sum() * (1.0 / norm), norm, self.rnnt_weight
        return out

    def rnnt_nll(self, enc_h, ys):
        """Per-utterance transducer negative log-likelihood [B] of the labels `ys` given the encoder output enc_h [B, T', H]
        of the forward that has just run (the frame lengths are the encoder's device copy): TransducerHead.nll."""
        if not hasattr(self, "rnnt"):
            raise ValueError("rnnt_nll needs the transducer head: build the model with rnnt_weight > 0")
        return self.rnnt.nll(enc_h, ys, self.encoder.enc2.last_lens_dev)

    def recognize_rnnt(self, xs, ilens, max_symbols=3, max_dec_timesteps=200):
        """Greedy decoding with the transducer head alone (not a reference method): the encoder and lin_enc
        once, then TransducerHead.greedy - at most max_symbols tokens per encoder frame, max_dec_timesteps in all, the lower
        index on ties.  -> one id list per utterance, as recognize_ctc returns them; self.last_rnnt keeps the device
        tensors of the call: dict(tokens int32 [B, max_dec_timesteps], lengths int32 [B], scores fp32 [B]: the sum of the
        emitted tokens' log-probabilities).  One host read, behind the loop."""
        if not hasattr(self, "rnnt"):
            raise ValueError("recognize_rnnt needs the transducer head: build the model with rnnt_weight > 0")
        if int(max_symbols) < 1 or int(max_dec_timesteps) < 1:
            raise ValueError("recognize_rnnt: max_symbols and max_dec_timesteps must be at least 1")
        if xs.is_cuda:
            hb.upload_side_stream_for(xs.shape[0] * xs.shape[1])
        with torch.no_grad():
            enc_h, _ = self.encoder(xs, ilens)
            out, n, score = self.rnnt.greedy(enc_h, self.encoder.enc2.last_lens_dev, int(max_symbols), int(max_dec_timesteps))
            host = torch.cat([n.view(-1, 1), out], dim=1).cpu().tolist()
        self.last_rnnt = dict(tokens=out, lengths=n, scores=score)
        return [row[1:1 + row[0]] for row in host]

    def recognize_rnnt_beams(self, xs, ilens, beam_size, max_dec_timesteps=200, ngram=None, ngram_weight=0.0, ngram_bonus=0.0,
                             eos_term=True, *, word_lm=None, word_lm_weight=0.0, word_bonus=0.0, lexicon_only=False):
        """Beam search with the transducer head alone (not a reference method): the encoder once, then
        TransducerHead.beam with `beam_size` entries and at most max_dec_timesteps labels; ngram (an ngram.NgramLM) sits inside
        the search by shallow fusion.  -> the id list of the best hypothesis per utterance; self.last_rnnt_beams keeps the
        device n-best of the call: dict(tokens int32 [B, beam, max_dec_timesteps] padded with -1, lengths int32 [B, beam] with
        -1 in unused slots, scores fp32 [B, beam] descending, parts: dict(rnnt, lm) with ngram, else empty).  With word_lm (a
        word_lm.WordLM) the lexicon and the word-level LM sit inside the search instead, weighed by word_lm_weight
        and word_bonus (per completed word), lexicon_only keeping only sequences of lexicon words: parts is dict(rnnt, lm) and
        n_words int32 [B, beam] joins the record.  One host read, behind the loop."""
        if not hasattr(self, "rnnt"):
            raise ValueError("recognize_rnnt_beams needs the transducer head: build the model with rnnt_weight > 0")
        if int(max_dec_timesteps) < 1:
            raise ValueError("recognize_rnnt_beams: max_dec_timesteps must be at least 1")
        if xs.is_cuda:
            hb.upload_side_stream_for(xs.shape[0] * xs.shape[1])
        with torch.no_grad():
            enc_h, _ = self.encoder(xs, ilens)
            out = self.rnnt.beam(enc_h, self.encoder.enc2.last_lens_dev, int(beam_size), int(max_dec_timesteps), ngram=ngram,
                                 ngram_weight=ngram_weight, ngram_bonus=ngram_bonus, eos_term=eos_term, word_lm=word_lm,
                                 word_lm_weight=word_lm_weight, word_bonus=word_bonus, lexicon_only=lexicon_only)
            hyp, hyp_len, score = out[:3]
            host = torch.cat([hyp_len[:, :1], hyp[:, 0]], dim=1).cpu().tolist()
        parts = dict(rnnt=out[3], lm=out[4]) if (ngram is not None or word_lm is not None) else {}
        self.last_rnnt_beams = dict(tokens=hyp, lengths=hyp_len, scores=score, parts=parts)
        if word_lm is not None:
            self.last_rnnt_beams["n_words"] = out[5]
        return [row[1:1 + max(row[0], 0)] for row in host]

    def ctc_nll(self, enc_h, ys):
        """Per-utterance CTC negative log-likelihood [B] of the labels `ys` given the encoder output enc_h [B, T', H] of the
        forward that has just run (the frame lengths are the encoder's device copy): ctc_lo over the B T' rows on the GEMM,
        then ops.ctc_loss on the raw logits.  An utterance with fewer frames than its labels need counts as 0
        (zero_infinity), like torch.nn.functional.ctc_loss(zero_infinity=True).  In training mode with
        self.ctc_star_penalty set: ops.ctc_star_loss with that penalty for every row instead."""
        bsz, frames, hid = enc_h.shape
        logits = ops.linear(enc_h.reshape(bsz * frames, hid), self.ctc_lo.weight, self.ctc_lo.bias).view(bsz, frames, -1)
        labels = torch.cat([y.reshape(-1) for y in ys]).to(device=enc_h.device, dtype=torch.long)
        ylens = [int(y.size(0)) for y in ys]
        if self.training and self.ctc_star_penalty is not None:
            return ops.ctc_star_loss(logits, self.encoder.enc2.last_lens_dev, labels, ylens, self.ctc_star_penalty, True)
        return ops.ctc_loss(logits, self.encoder.enc2.last_lens_dev, labels, ylens, True)

    def gtc_nll(self, enc_h, graphs):
        """Per-utterance graph CTC negative log path sum [B] (not a reference method) of the label graphs
        `graphs` - one gtc.Graph for every row or a gtc.GraphBatch naming a graph per row - given the encoder output enc_h
        [B, T', H] of the forward that has just run: ctc_lo over the B T' rows on the GEMM, then ops.gtc_loss on the raw
        logits.  A row whose graph has no path of its frame count counts as 0 (zero_infinity), like ctc_nll.  The value is a
        path sum, not a normalised probability; no gradient flows to the graph's weights.  `graphs` may also be the
        gtc.DeviceGraphTable of ops.gtc_nbest_graphs."""
        if not hasattr(self, "ctc_lo"):
            raise ValueError("gtc_nll needs the CTC head: build the model with ctc_weight > 0")
        bsz, frames, hid = enc_h.shape
        logits = ops.linear(enc_h.reshape(bsz * frames, hid), self.ctc_lo.weight, self.ctc_lo.bias).view(bsz, frames, -1)
        return ops.gtc_loss(logits, self.encoder.enc2.last_lens_dev, graphs, True)

    def recognize_beams(self, data, ilens, max_dec_timesteps, topk, length_penalty=0.0, nbest=False, *, lm=None,
                        lm_weight=0.0, ctc_decode_weight=0.0, ngram=None, ngram_weight=0.0, ngram_bonus=0.0, word_lm=None,
                        word_lm_weight=0.0, word_bonus=0.0, lexicon_only=False):
        """Encoder, then Decoder.recognize_beams (not a reference method).  ngram / word_lm: the n-gram or the
        lexicon and word-level LM inside the search, as the decoder's method takes them; self.last_beams keeps the device record
        of such a call - dict(tokens, lengths, scores, parts: dict(att, lm), n_words) - in the style of last_rnnt_beams.  ctc_decode_weight in (0, 1]: joint CTC-attention
        decoding with the model's CTC head - it needs a model built with ctc_weight > 0; the weight of the
        training loss (self.ctc_weight) and this one are separate."""
        ctc_decode_weight = float(ctc_decode_weight)
        if not 0.0 <= ctc_decode_weight <= 1.0:
            raise ValueError("ctc_decode_weight must lie in [0, 1], got %r" % (ctc_decode_weight,))
        if ctc_decode_weight > 0 and not hasattr(self, "ctc_lo"):
            raise ValueError("ctc_decode_weight %g needs the CTC head: build the model with ctc_weight > 0" % ctc_decode_weight)
        self.decoder.check_ngram(ngram)
        self.decoder.check_word_lm(word_lm, ngram)
        table_lm = {}
        if ngram is not None or word_lm is not None:
            table_lm = dict(ngram=ngram, ngram_weight=ngram_weight, ngram_bonus=ngram_bonus, word_lm=word_lm,
                            word_lm_weight=word_lm_weight, word_bonus=word_bonus, lexicon_only=lexicon_only)
        if data.is_cuda:
            hb.upload_side_stream_for(data.shape[0] * data.shape[1])
        with torch.no_grad():
            enc_h, enc_lens = self.encoder(data, ilens)
            ctc_logits = ctc_lens = None
            if ctc_decode_weight > 0:                  # the product ctc_nll forms, on the frames the decoder attends to
                bsz, frames, hid = enc_h.shape
                ctc_logits = ops.linear(enc_h.reshape(bsz * frames, hid), self.ctc_lo.weight, self.ctc_lo.bias).view(bsz, frames, -1)
                ctc_lens = self.encoder.enc2.last_lens_dev
            out = self.decoder.recognize_beams(enc_h, enc_lens, max_dec_timesteps, topk, length_penalty=length_penalty,
                                               nbest=nbest, lm=lm, lm_weight=lm_weight, ctc_logits=ctc_logits,
                                               ctc_lens=ctc_lens, ctc_decode_weight=ctc_decode_weight, **table_lm)
            self.last_beams = self.decoder.last_beams
            return out

    @property
    def time_reduction(self):
        """Input frames per encoder frame (an integer, from the encoder's own layers): encoder frame t of `align` covers the
        input frames t * time_reduction .. (t + 1) * time_reduction - 1, and an utterance of n input frames has
        ceil(n / time_reduction) encoder frames."""
        return self.encoder.enc2.time_reduction

    def _ctc_logits(self, data, ilens, what):
        """Encoder, then ctc_lo on the rows ctc_nll uses -> (raw CTC logits [B, T', V], the frame lengths on the device, and
        on the host).  Without the head: ValueError before any launch."""
        return self._encode_ctc(data, ilens, what)[:3]

    def _encode_ctc(self, data, ilens, what):
        """_ctc_logits with the encoder output behind it: (logits, frame lengths on the device, on the host, enc_h)."""
        if not hasattr(self, "ctc_lo"):
            raise ValueError("%s needs the CTC head: build the model with ctc_weight > 0" % what)
        if data.is_cuda:
            hb.upload_side_stream_for(data.shape[0] * data.shape[1])
        enc_h, enc_lens = self.encoder(data, ilens)
        bsz, frames, hid = enc_h.shape
        logits = ops.linear(enc_h.reshape(bsz * frames, hid), self.ctc_lo.weight, self.ctc_lo.bias).view(bsz, frames, -1)
        return logits, self.encoder.enc2.last_lens_dev, enc_lens, enc_h

    def align(self, xs, ilens, ys):
        """CTC forced alignment of the transcripts `ys` (a list of label tensors, as forward takes them) to the utterances
        (not a reference method): encoder, the CTC head, ops.ctc_align.  -> one dict per utterance:
        tokens (the label ids), first / last (the inclusive ENCODER frames of each token; times time_reduction for input
        frames), confidence (exp(token_logp / (last - first + 1)): the geometric mean of the head's frame posteriors of the
        token over its frames), score (the log-probability of the best alignment; -inf: the transcript does not fit the
        frames - then first = last = -1 and the confidences are 0) and frames (the utterance's encoder frames).  The device
        results are read once."""
        with torch.no_grad():
            logits, lens_dev, enc_lens = self._ctc_logits(xs, ilens, "align")
            labels = torch.cat([y.reshape(-1) for y in ys]).to(device=logits.device, dtype=torch.long)
            counts = [int(y.numel()) for y in ys]
            res = ops.ctc_align(logits, lens_dev, labels, counts)
            span = (res.last - res.first + 1).clamp(min=1).to(torch.float32)
            conf = torch.exp(res.token_logp / span)
            # one read: [first, last, confidence, labels] per label, then the scores
            packed = torch.cat([res.first.double(), res.last.double(), conf.double(), labels.double(), res.score.double()]).cpu()
        n = labels.numel()
        first, last, conf, toks, score = (packed[:n].long().tolist(), packed[n:2 * n].long().tolist(), packed[2 * n:3 * n].tolist(),
                                          packed[3 * n:4 * n].long().tolist(), packed[4 * n:].tolist())
        out, o = [], 0
        for b, c in enumerate(counts):
            out.append(dict(tokens=toks[o:o + c], first=first[o:o + c], last=last[o:o + c], confidence=conf[o:o + c],
                            score=score[b], frames=int(enc_lens[b])))
            o += c
        self.last_alignment = res                                # (the device tensors of the call, path included)
        return out

    def segment(self, xs, ilens, texts, window=30):
        """CTC segmentation of recordings against their transcripts (not a reference method): encoder, the CTC
        head, ops.ctc_segment with free ends.  `texts` is a list, per recording, of label tensors, one per utterance.  -> one
        dict per recording: score (the log-probability of the text over the frames it picks; -inf: it does not fit), frames
        (the recording's encoder frames) and utterances, a list of dicts: tokens (the label ids), begin / end (inclusive
        ENCODER frames; times time_reduction for input frames; -1 without labels or when the text does not fit), logp (the
        path's log-probability over begin .. end) and confidence (the lowest mean of the path's frame log-probabilities over
        the consecutive blocks of `window` frames: one bad stretch sinks it).  The recording goes through the encoder in one
        pass.  self.last_segmentation keeps the device result (ops.CtcSegmentation).  One host read."""
        with torch.no_grad():
            logits, lens_dev, enc_lens = self._ctc_logits(xs, ilens, "segment")
            flat = [y.reshape(-1) for rec in texts for y in rec]
            labels = (torch.cat(flat) if flat else torch.zeros(0)).to(device=logits.device, dtype=torch.long)
            counts = [[int(y.numel()) for y in rec] for rec in texts]
            res = ops.ctc_segment(logits, lens_dev, labels, counts, free_ends=True, window=window)
            # one read: [begin, end, logp, confidence] per utterance, then the labels and the scores
            packed = torch.cat([res.utt_begin.double(), res.utt_end.double(), res.utt_logp.double(), res.utt_conf.double(),
                                labels.double(), res.score.double()]).cpu()
        n = sum(len(rec) for rec in counts)
        begin, end = packed[:n].long().tolist(), packed[n:2 * n].long().tolist()
        logp, conf = packed[2 * n:3 * n].tolist(), packed[3 * n:4 * n].tolist()
        toks, score = packed[4 * n:4 * n + labels.numel()].long().tolist(), packed[4 * n + labels.numel():].tolist()
        out, u, o = [], 0, 0
        for b, rec in enumerate(counts):
            utts = []
            for c in rec:
                utts.append(dict(tokens=toks[o:o + c], begin=begin[u], end=end[u], logp=logp[u], confidence=conf[u]))
                u += 1
                o += c
            out.append(dict(score=score[b], frames=int(enc_lens[b]), utterances=utts))
        self.last_segmentation = res
        return out

    def align_rnnt(self, xs, ilens, ys):
        """Forced alignment of the transcripts `ys` (a list of label tensors, as forward takes them) to the utterances with
        the transducer head (not a reference method): encoder, TransducerHead.logits, ops.rnnt_align.  -> one
        dict per utterance: tokens (the label ids), frame (the ENCODER frame on which each token is emitted; times
        time_reduction for input frames), confidence (exp(token_logp): the head's posterior of the token at its node; 0 on
        a row that cannot be aligned, whose frames are -1), score (the log-probability of the best alignment; -inf: not
        aligned) and frames (the utterance's encoder frames).  self.last_rnnt_alignment keeps the device result
        (ops.RnntAlignment).  One host read."""
        if not hasattr(self, "rnnt"):
            raise ValueError("align_rnnt needs the transducer head: build the model with rnnt_weight > 0")
        if xs.is_cuda:
            hb.upload_side_stream_for(xs.shape[0] * xs.shape[1])
        with torch.no_grad():
            enc_h, enc_lens = self.encoder(xs, ilens)
            lens_dev = self.encoder.enc2.last_lens_dev
            labels = torch.cat([y.reshape(-1) for y in ys]).to(device=enc_h.device, dtype=torch.long)
            counts = [int(y.numel()) for y in ys]
            res = ops.rnnt_align(self.rnnt.logits(enc_h, ys, lens_dev), lens_dev, labels, counts)
            # one read: [frame, confidence, label] per label, then the scores
            packed = torch.cat([res.emit_frame.double(), torch.exp(res.token_logp).double(), labels.double(),
                                res.score.double()]).cpu()
        n = labels.numel()
        frame, conf, toks, score = (packed[:n].long().tolist(), packed[n:2 * n].tolist(), packed[2 * n:3 * n].long().tolist(),
                                    packed[3 * n:].tolist())
        out, o = [], 0
        for b, c in enumerate(counts):
            out.append(dict(tokens=toks[o:o + c], frame=frame[o:o + c], confidence=conf[o:o + c], score=score[b],
                            frames=int(enc_lens[b])))
            o += c
        self.last_rnnt_alignment = res
        return out

    def recognize_ctc(self, xs, ilens):
        """Best-path decoding with the CTC head alone (not a reference method): the argmax token of every
        encoder frame, repeats collapsed, blanks dropped (ops.ctc_greedy) -> one id list per utterance."""
        with torch.no_grad():
            logits, lens_dev, _ = self._ctc_logits(xs, ilens, "recognize_ctc")
            ids, n, frame_tok = ops.ctc_greedy(logits, lens_dev)
            host = torch.cat([n.view(-1, 1), ids], dim=1).cpu().tolist()
        self.last_frame_tokens = frame_tok
        return [row[1:1 + row[0]] for row in host]

    @staticmethod
    def _beam_width(topk):
        K = int(topk)
        if not 1 <= K <= hb.BEAM_KMAX:
            raise ValueError("beam width %d outside 1..%d" % (K, hb.BEAM_KMAX))
        return K

    def recognize_ctc_beams(self, xs, ilens, topk, nbest=False, *, ngram=None, ngram_weight=0.0, ngram_bonus=0.0, word_lm=None,
                            word_lm_weight=0.0, word_bonus=0.0, lexicon_only=False, eos_term=True, context=None, ctx_weight=1.0):
        """CTC prefix beam search with the CTC head alone (not a reference method): encoder, the head,
        ops.ctc_beam with beam width topk (1..16) -> (ids, scores): per utterance the best label sequence (an id list) and
        its log-mass; with nbest=True per utterance the ranked list of all hypotheses the search kept (at most topk) and
        the list of their scores.  The device results are read once.
        With ngram (an ngram.NgramLM over the decoder's vocabulary) the LM sits inside the search: hypotheses
        rank by (log-mass + ngram_weight lm) + ngram_bonus len with the LM's end-of-sentence term, and the scores are
        those ranks; self.last_ctc_beams then also holds ctc_score and lm_score.
        With word_lm (a word_lm.WordLM spelled in the decoder's vocabulary) the lexicon and the word LM sit
        inside the search: hypotheses rank by (log-mass + word_lm_weight lm) + word_bonus n_words, lexicon_only keeps only
        sequences of lexicon words (an utterance may then keep no hypothesis: an empty list; without nbest the empty id
        list at -inf); self.last_ctc_beams then holds ctc_score, lm_score and n_words too.
        With context (a context.ContextGraph for every utterance, or a context.ContextBatch naming a graph per utterance;
        DESIGN 4.32) the phrase lists sit inside the search, alone or beside ngram: a hypothesis ranks by its rank without a
        context plus ctx_weight bias; self.last_ctc_beams then ends with ctx_score, the bias of every hypothesis."""
        K = self._beam_width(topk)
        self.decoder.check_ngram(ngram)
        self.decoder.check_context(context, word_lm)
        self.decoder.check_word_lm(word_lm, ngram)
        with torch.no_grad():
            logits, lens_dev, _ = self._ctc_logits(xs, ilens, "recognize_ctc_beams")
            if context is not None:
                beams = ops.ctc_beam(logits, lens_dev, K, ngram=ngram, ngram_weight=ngram_weight, ngram_bonus=ngram_bonus,
                                     eos_term=True, context=context, ctx_weight=ctx_weight)
                hyp, hyp_len, score = beams[:3]
            elif word_lm is not None:
                beams = ops.ctc_beam(logits, lens_dev, K, word_lm=word_lm, word_lm_weight=word_lm_weight, word_bonus=word_bonus,
                                     lexicon_only=lexicon_only, eos_term=eos_term)
                hyp, hyp_len, score = beams[:3]
            elif ngram is None:
                hyp, hyp_len, score = beams = ops.ctc_beam(logits, lens_dev, K)
            else:
                beams = ops.ctc_beam(logits, lens_dev, K, ngram=ngram, ngram_weight=ngram_weight, ngram_bonus=ngram_bonus,
                                     eos_term=True)
                hyp, hyp_len, score = beams[:3]
            bsz, _, T = hyp.shape
            host = torch.cat([hyp_len.view(bsz, K, 1).double(), score.view(bsz, K, 1).double(), hyp.double()], dim=2).cpu().tolist()
        self.last_ctc_beams = tuple(beams)                       # (the device tensors of the call)
        ids = [[[int(v) for v in row[2:2 + int(row[0])]] for row in utt if row[0] >= 0] for utt in host]
        scores = [[row[1] for row in utt if row[0] >= 0] for utt in host]
        if nbest:
            return ids, scores
        if word_lm is not None:                                  # (lexicon_only may leave an utterance without a hypothesis)
            return [u[0] if u else [] for u in ids], [u[0] if u else float("-inf") for u in scores]
        return [u[0] for u in ids], [u[0] for u in scores]

    def ctc_beams_on_device(self, xs, ilens, topk, *, ngram=None, ngram_weight=0.0, ngram_bonus=0.0):
        """recognize_ctc_beams without its host read (not a reference method): encoder, the head, ops.ctc_beam
        with beam width topk (with ngram inside, as there) -> (hyp int32 [B, topk, T'], hyp_len int32 [B, topk], score fp32
        [B, topk]) on the device, for ops.gtc_nbest_graphs.  Nothing is read back."""
        K = self._beam_width(topk)
        self.decoder.check_ngram(ngram)
        with torch.no_grad():
            logits, lens_dev, _ = self._ctc_logits(xs, ilens, "ctc_beams_on_device")
            if ngram is None:
                beams = ops.ctc_beam(logits, lens_dev, K)
            else:
                beams = ops.ctc_beam(logits, lens_dev, K, ngram=ngram, ngram_weight=ngram_weight, ngram_bonus=ngram_bonus,
                                     eos_term=True)
        self.last_ctc_beams = tuple(beams)
        return beams[0], beams[1], beams[2]

    def word_lm_score(self, word_lm, ids, eos_term=True):
        """The word LM's log-probability (ops.word_lm_score) of hypotheses this model produced, to rescore any
        list with: ids as E2E.ngram_score takes them (a device tensor [..., L], <EOS>-padded, a row counting up to its first
        <EOS> - or a list of id lists).  -> (fp32 [...] scores, int32 [...] numbers of words) on the device."""
        self.decoder.check_word_lm(word_lm)
        if not isinstance(ids, torch.Tensor):
            rows = [[int(c) for c in row] for row in ids]
            L = max([len(r) for r in rows] + [1])
            dev = next(self.parameters()).device
            flat = torch.tensor([r + [self.decoder.eos] * (L - len(r)) for r in rows], dtype=torch.int32).to(dev)
            lens = hb.to_device_i32([len(r) for r in rows], dev)
            return ops.word_lm_score(word_lm, flat, lens, eos_term=eos_term)
        L = ids.shape[-1]
        flat = ids.reshape(-1, L)
        is_eos = flat == self.decoder.eos
        first = torch.where(is_eos.any(dim=1), is_eos.to(torch.int32).argmax(dim=1), torch.full_like(flat[:, 0], L)).to(torch.int32)
        score, n_words = ops.word_lm_score(word_lm, flat, first, eos_term=eos_term)
        return score.view(ids.shape[:-1]), n_words.view(ids.shape[:-1])

    def context_score(self, context, ids, graph_of=None):
        """The bias (ops.context_score) of hypotheses this model produced under a context.ContextGraph or
        ContextBatch: ids as E2E.ngram_score takes them (a device tensor [..., L], <EOS>-padded, a row counting up to its
        first <EOS> - or a list of id lists); graph_of: the graph of every row (a list or an int32 tensor; None: the
        context's own list, or its one graph).  -> fp32 [...] on the device."""
        self.decoder.check_context(context)
        dev = next(self.parameters()).device
        if graph_of is not None and not isinstance(graph_of, torch.Tensor):
            graph_of = hb.to_device_i32([int(g) for g in graph_of], dev)
        if not isinstance(ids, torch.Tensor):
            rows = [[int(c) for c in row] for row in ids]
            L = max([len(r) for r in rows] + [1])
            flat = torch.tensor([r + [self.decoder.eos] * (L - len(r)) for r in rows], dtype=torch.int32).to(dev)
            lens = hb.to_device_i32([len(r) for r in rows], dev)
            return ops.context_score(context, flat, lens, graph_of=graph_of)
        L = ids.shape[-1]
        flat = ids.reshape(-1, L)
        is_eos = flat == self.decoder.eos
        first = torch.where(is_eos.any(dim=1), is_eos.to(torch.int32).argmax(dim=1), torch.full_like(flat[:, 0], L)).to(torch.int32)
        return ops.context_score(context, flat, first, graph_of=graph_of).view(ids.shape[:-1])

    def ngram_score(self, ngram, ids, eos_term=True):
        """The n-gram LM's log-probability (ops.ngram_score) of hypotheses this model produced, to rescore any
        list with: ids a device tensor [..., L] of label ids, <EOS>-padded as recognize_beams(nbest=True) and
        recognize_two_pass return them (a row counts up to its first <EOS>) - or a list of id lists.  -> fp32 [...] on the
        device (a list: [N]), the end-of-sentence term included when eos_term.  No host read for a tensor."""
        self.decoder.check_ngram(ngram)
        if not isinstance(ids, torch.Tensor):
            rows = [[int(c) for c in row] for row in ids]
            L = max([len(r) for r in rows] + [1])
            dev = next(self.parameters()).device
            flat = torch.tensor([r + [self.decoder.eos] * (L - len(r)) for r in rows], dtype=torch.int32).to(dev)
            lens = hb.to_device_i32([len(r) for r in rows], dev)
            return ops.ngram_score(ngram, flat, lens, eos_term=eos_term)
        L = ids.shape[-1]
        flat = ids.reshape(-1, L)
        is_eos = flat == self.decoder.eos
        first = torch.where(is_eos.any(dim=1), is_eos.to(torch.int32).argmax(dim=1), torch.full_like(flat[:, 0], L)).to(torch.int32)
        return ops.ngram_score(ngram, flat, first, eos_term=eos_term).view(ids.shape[:-1])

    def recognize_two_pass(self, xs, ilens, topk, ctc_weight=0.5, length_penalty=0.0, nbest=False, *, lm=None, lm_weight=0.0,
                           ngram=None, ngram_weight=0.0, ngram_bonus=0.0, word_lm=None, word_lm_weight=0.0, word_bonus=0.0,
                           lexicon_only=False, eos_term=True, context=None, ctx_weight=1.0):
        """Two-pass decoding (not a reference method): the CTC prefix beam search of the head proposes topk
        (1..16) hypotheses per utterance, ONE teacher-forced pass of the attention decoder over the B topk rows scores them
        (Decoder.score_hypotheses), and with lm (an LM module) and lm_weight != 0 one teacher-forced pass of the LM too.
        Hypothesis k of utterance b scores ((1 - w) att + w ctc + lm_weight lm) / (len + 1)**length_penalty with w =
        ctc_weight in [0, 1]: fp32, every operation rounded on its own, in this order; att and lm are sums of token
        log-probabilities, <EOS> included, ctc the search's log-mass.  Ranked per utterance, ties to the search's order; a
        slot the search left unused stays at -inf.
        -> (prediction [B, L] int64, scores [B]): the best hypothesis, <EOS>-padded to L = T' + 1; with nbest=True all topk,
        ranked: ([B, topk, L], [B, topk]) - the shapes of recognize_beams.  Device tensors: no host read in here, and none
        between the passes.  self.last_two_pass keeps the parts (hyp, hyp_len, ctc, att, lm, order).
        With ngram (an ngram.NgramLM) the first pass is the search with the LM inside, and the score is
        ((1 - w) att + w ctc + lm_weight lm + ngram_weight lm_ngram + ngram_bonus len) / (len + 1)**length_penalty, in this
        order, with ctc the search's ctc_score and lm_ngram its lm_score (parts: also ngram and rank).
        With word_lm (a word_lm.WordLM) the first pass is the search with the lexicon and the word LM inside, and
        the score gains + word_lm_weight lm_word + word_bonus n_words where the n-gram term stands, before the length
        penalty (parts: also word_lm, n_words and rank).
        With context (a context.ContextGraph or ContextBatch) the first pass searches with the phrase lists
        inside, alone or beside ngram, and the score gains + ctx_weight ctx_score behind the n-gram term (parts: also
        context and rank)."""
        K = self._beam_width(topk)
        w = float(ctc_weight)
        if not 0.0 <= w <= 1.0:
            raise ValueError("ctc_weight must lie in [0, 1], got %r" % (ctc_weight,))
        dec = self.decoder
        dec.check_lm(lm)
        dec.check_ngram(ngram)
        dec.check_context(context, word_lm)
        dec.check_word_lm(word_lm, ngram)
        extra = {} if ngram is None else dict(ngram=ngram, ngram_weight=ngram_weight, ngram_bonus=ngram_bonus)
        if word_lm is not None:
            extra = dict(word_lm=word_lm, word_lm_weight=word_lm_weight, word_bonus=word_bonus, lexicon_only=lexicon_only,
                         eos_term=eos_term)
        if context is not None:
            extra.update(context=context, ctx_weight=ctx_weight)
        with torch.no_grad():
            logits, lens_dev, enc_lens, enc_h = self._encode_ctc(xs, ilens, "recognize_two_pass")
            tokens, scores, parts = dec.rescore_ctc_beams(enc_h, enc_lens, logits, lens_dev, K, ctc_weight=w,
                                                          length_penalty=length_penalty, lm=lm, lm_weight=lm_weight, **extra)
        self.last_two_pass = parts
        if nbest:
            return tokens, scores
        return tokens[:, 0], scores[:, 0]

    MWER_EXTRA_STEPS = 5          # the n-best search of an MWER step runs at most this many steps past the longest reference
    space_id = None               # the id of <space>, set by the Solver: what mwer_forward(unit="word") splits words at

    def mwer_forward(self, xs, ilens, ys, beam, ce_weight=0.01, max_dec_timesteps=200, hyps=None, unit="token"):
        """The loss of one minimum-error-rate training step (not a reference method; DESIGN 4.20, Prabhavalkar et al. 2018):
        L_mwer + ce_weight L_ce with L_mwer = mean_b sum_k phat_k (err_k - mean err) over the `beam` (1..16) hypotheses of the
        n-best list, phat the model's sequence probabilities renormalised over the list.
          the encoder runs once, in the module's mode;
          under no_grad Decoder.recognize_beams(nbest=True) on that output, min(max_dec_timesteps, longest reference +
            MWER_EXTRA_STEPS) steps - or `hyps` = (tokens int [B, beam, T] <EOS>-padded, lengths int32 [B, beam] or None: up to
            the first <EOS>; < 0: an unused slot) instead of the search;
          hb.edit_distance of the B beam hypotheses (cut at <EOS>, nothing filtered) to the B references - with unit="word"
            hb.word_edit_distance at self.space_id: err counts word errors, nothing else changes;
          Decoder.score_hypotheses_grad and ops.mwer_loss with scale = 1 / B;
          with ce_weight > 0 the supervised loss of E2E.forward on the same encoder output (teacher-forced, label smoothing
            and dropout as there, the CTC term when ctc_weight > 0).
        -> the loss, a device scalar.  self.last_mwer keeps the parts: tokens, hyp_len, err, npos, seq_logp, post, risk, coef,
        mwer, ce.  Nothing is read on the host."""
        K = self._beam_width(beam)
        if unit not in ("token", "word"):
            raise ValueError("mwer_forward: unit %r is neither 'token' nor 'word'" % (unit,))
        if unit == "word" and self.space_id is None:
            raise ValueError("mwer_forward(unit='word') needs E2E.space_id, the id of <space>")
        if xs.is_cuda:
            hb.upload_side_stream_for(xs.shape[0] * xs.shape[1])
        enc_h, enc_lens = self.encoder(xs, ilens)
        dec = self.decoder
        bsz, dev = enc_h.shape[0], enc_h.device
        with torch.no_grad():
            if hyps is None:
                steps = max(1, min(int(max_dec_timesteps), max(int(y.size(0)) for y in ys) + self.MWER_EXTRA_STEPS))
                tokens, scores = dec.recognize_beams(enc_h.detach(), enc_lens, steps, K, nbest=True)
                hyp_len = None
                unused = scores == float("-inf")                  # a rank the search left without a hypothesis
            else:
                tokens, hyp_len = hyps
                if tuple(tokens.shape[:2]) != (bsz, K):
                    raise ValueError("hyps: tokens %s are not [%d utterances, %d hypotheses, T]" % (tuple(tokens.shape), bsz, K))
                unused = None if hyp_len is None else hyp_len < 0
            T = tokens.shape[2]
            to_eos = ((tokens == dec.eos).to(torch.int32).cumsum(dim=2) == 0).sum(dim=2).to(torch.int32)     # tokens before <EOS>
            hyp_len = to_eos if hyp_len is None else torch.minimum(hyp_len.to(torch.int32), to_eos)
            if unused is not None:
                hyp_len = torch.where(unused, torch.full_like(hyp_len, -1), hyp_len)
            ref = dec._label_matrices(ys)[1].to(torch.int32).contiguous()       # [B, longest + 1]: <EOS>-padded, read to ref_len
            ref_len = hb_to_device([int(y.size(0)) for y in ys], dev)
            ref_index = (torch.arange(bsz * K, device=dev, dtype=torch.int32) // K).int()
            pairs = dict(hyp_len=hyp_len.reshape(-1).clamp(min=0), ref_index=ref_index, eos=dec.eos)
            if unit == "word":
                err, _, _ = hb.word_edit_distance(tokens.reshape(bsz * K, T), ref, ref_len, int(self.space_id), **pairs)
            else:
                err, _, _ = hb.edit_distance(tokens.reshape(bsz * K, T), ref, ref_len, **pairs)
        _, logits, tok_out_lb, npos = dec.score_hypotheses_grad(enc_h, enc_lens, tokens, hyp_len, scores=False)
        mwer, parts = ops.mwer_loss(logits, tok_out_lb, npos, err, 1.0 / bsz, n_utts=bsz)
        loss, ce = mwer, None
        if float(ce_weight) > 0:
            lp = dec(enc_h, enc_lens, ys, loss_norm=bsz)[1]
            ce = lp.fused_loss                                   # -sum(log-probs) / (B olength): E2E.forward's loss
            if self.ctc_weight > 0:
                ce = (1.0 - self.ctc_weight) * ce + self.ctc_weight * (self.ctc_nll(enc_h, ys).sum() * (1.0 / bsz))
            loss = mwer + float(ce_weight) * ce
        self.last_mwer = dict(parts, tokens=tokens, hyp_len=hyp_len, err=err, npos=npos, mwer=mwer.detach(),
                              ce=None if ce is None else ce.detach())
        return loss

    def mask_and_cal_loss(self, log_probs, ys, mask=None):
        if mask is None:
            seq_len = [y.size(0) + 1 for y in ys]              # +1 for <EOS>
            mask = _seq_mask(seq_len=seq_len, max_len=log_probs.size(1)).to(log_probs.device)
        else:
            seq_len = [y.size(0) for y in ys]
        return -torch.sum(log_probs * mask) / sum(seq_len)


class LM(torch.nn.Module):
    """The judge: 2-layer LSTM language model (model.py:459-573) on the same fused LSTM kernel."""

    def __init__(self, output_dim, embedding_dim, hidden_dim, dropout_rate, n_layers, bos, eos, pad, ls_weight,
                 labeldist):
        super(LM, self).__init__()
        self.bos, self.eos, self.pad = bos, eos, pad
        self.embedding = torch.nn.Embedding(output_dim, embedding_dim, padding_idx=pad)
        self.LSTM = _LstmWeights(embedding_dim, hidden_dim, num_layers=n_layers, bidirectional=False)
        # re-init as utils.weight_init does for nn.LSTM (utils.py:97-103): orthogonal matrices, normal biases
        for prm in self.LSTM.parameters():
            if prm.dim() >= 2:
                torch.nn.init.orthogonal_(prm.data)
            else:
                torch.nn.init.normal_(prm.data)
        self.output_layer = torch.nn.Linear(hidden_dim, output_dim)
        self.dropout_layer = torch.nn.Dropout(p=dropout_rate)
        self.hidden_dim, self.output_dim = hidden_dim, output_dim
        self.dropout_rate, self.n_layers = dropout_rate, n_layers
        self.ls_weight = ls_weight
        self.labeldist = labeldist
        self._dist_dev = {}
        if labeldist is not None:
            self.vlabeldist = cc(torch.from_numpy(np.array(labeldist, dtype=np.float32)))

    def _run_lstm(self, x_tm, lens_dev):
        """x_tm [T,B,E] -> [T,B,H] through all layers; inter-layer dropout like nn.LSTM(dropout=p)."""
        packs = ops.lstm_pack([self.LSTM.direction_params(l) for l in range(self.n_layers)], 1)    # all layers: one launch
        for l in range(self.n_layers):
            x_tm = ops.lstm_layer(x_tm, lens_dev, None, 1, packed=packs[l])
            if l + 1 < self.n_layers and self.training and self.dropout_rate > 0:
                x_tm = F.dropout(x_tm, self.dropout_rate, True)
        return x_tm

    def forward(self, ys=None, discrete_input=True):
        """-> (ys_log_probs, ys_probs, predictions), each [B,L] (model.py:492-532)."""
        dev = self.embedding.weight.device
        if discrete_input:
            bos = ys[0].new_tensor([self.bos])
            eos = ys[0].new_tensor([self.eos])
            seq_in = [torch.cat([bos, y, eos, eos, eos, eos]) for y in ys]
            seq_out = [torch.cat([y, eos, eos, eos, eos, eos]) for y in ys]
            tok_in = pad_list(seq_in, self.eos).to(dev)
            tok_out = pad_list(seq_out, self.eos).to(dev)
            lens = [int(s.size(0)) for s in seq_in]
        else:
            first = torch.full((ys.size(0), 1), self.bos, dtype=ys.dtype, device=ys.device)
            tok_in = torch.cat([first, ys[:, :-1]], dim=1).to(dev)
            tok_out = ys.to(dev)
            lens = [tok_in.size(1)] * tok_in.size(0)
        eys = self.dropout_layer(self.embedding(tok_in))
        lens_dev = hb_to_device(lens, dev)
        out = self._run_lstm(eys.transpose(0, 1).contiguous(), lens_dev).transpose(0, 1)
        out = self.dropout_layer(out)
        logits = ops.linear(out.contiguous(), self.output_layer.weight, self.output_layer.bias)
        # log_softmax -> gather -> label smoothing (model.py:523-531) on the decoder's kernel (asr_label_logprob_*)
        plain, predictions = ops.label_logprob(logits, tok_out, with_argmax=True)      # log p(target); argmax of the logits
        ys_probs = plain.exp()
        if self.ls_weight > 0 and self.training:
            if str(dev) not in self._dist_dev:
                self._dist_dev[str(dev)] = self.vlabeldist.to(dev).float().contiguous()
            ys_log_probs = ops.label_logprob(logits, tok_out, self._dist_dev[str(dev)], self.ls_weight)
        else:
            ys_log_probs = plain
        return ys_log_probs, ys_probs, predictions

    def zero_state(self, ref, dim=None):
        """model.py:486-490."""
        return ref.new_zeros(self.n_layers, ref.size(0), dim if dim else self.hidden_dim)

    def forward_step(self, emb, dec_z=None, dec_c=None):
        """One step of the stacked LSTM + output layer with carried state (model.py:534-542; decode stage only, no
        autograd): emb [B, 1, E], dec_z / dec_c [n_layers, B, H] or None -> (logit [B, V], dec_z, dec_c).  The products
        run on asr_gemm_f32; inter-layer dropout as nn.LSTM(dropout=p) applies it (training mode only)."""
        with torch.no_grad():
            x = emb.reshape(emb.size(0), -1).contiguous()
            if dec_z is None:
                dec_z, dec_c = self.zero_state(x), self.zero_state(x)
            new_z, new_c = [], []
            for l in range(self.n_layers):
                w_ih, w_hh, b_ih, b_hh = self.LSTM.direction_params(l)
                gates = hb.gemm(x, w_ih, trans_b=True, bias=b_ih)
                hb.gemm(dec_z[l].contiguous(), w_hh, trans_b=True, bias=b_hh, out=gates, accumulate=True)
                gi, gf, gg, go = gates.chunk(4, dim=1)
                cl = torch.sigmoid(gf) * dec_c[l] + torch.sigmoid(gi) * torch.tanh(gg)
                zl = torch.sigmoid(go) * torch.tanh(cl)
                new_z.append(zl)
                new_c.append(cl)
                x = zl
                if l + 1 < self.n_layers and self.training and self.dropout_rate > 0:
                    x = F.dropout(x, self.dropout_rate, True)
            logit = hb.gemm(x.contiguous(), self.output_layer.weight, trans_b=True, bias=self.output_layer.bias)
        return logit, torch.stack(new_z), torch.stack(new_c)

    def decode(self, n_samples=5, sample=False, max_dec_timesteps=500):
        """Free-running generation with carried state (model.py:544-563; lm_validation's samples)."""
        dev = self.embedding.weight.device
        prev = torch.full((n_samples,), self.bos, dtype=torch.long, device=dev)
        dec_z = dec_c = None
        preds = []
        with torch.no_grad():
            for t in range(max_dec_timesteps):
                logit, dec_z, dec_c = self.forward_step(self.embedding(prev).unsqueeze(1), dec_z, dec_c)
                prev = torch.distributions.Categorical(logits=logit).sample() if sample else logit.argmax(-1)
                preds.append(prev)
        return torch.stack(preds, dim=1)

    def mask_and_cal_sum(self, log_probs, ys, mask=None):
        if mask is None:
            seq_len = [y.size(0) + 1 + 4 for y in ys]
            mask = _seq_mask(seq_len=seq_len, max_len=log_probs.size(1)).to(log_probs.device)
        else:
            seq_len = [y.size(0) for y in ys]
        return torch.sum(log_probs * mask) / sum(seq_len)
