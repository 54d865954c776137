"""The front end: packed waveforms -> the [B, T_max, D] features the encoder reads, on the GPU (csrc/frontend.hip).

Kaldi-convention log-mel filterbank energies (dither off, snip-edges), then - in dump.sh's order - CMVN, deltas and, in
training feeds, SpecAugment masks; rows behind an utterance are exact zeros.  Three launches (fbank; the per-utterance
statistics, in `utterance` mode only; the finish pass), no host synchronisation: every frame count follows from a sample
count, which the host has.  There is no CPU path.

Speed perturbation (csrc/resample.hip; training feeds only) is a fourth launch IN FRONT of the fbank: every
utterance is resampled by a factor drawn on the host (`draw_speed`: one generator per row of the batch in collated order),
so the host knows every perturbed sample count (`perturbed_samples`) and frame count before anything is uploaded; the fbank
then reads the resampled float32 buffer.  A factor of exactly 1 copies the samples by value.

Config (the `frontend` sub-dictionary; not a reference key):
  sample_rate 16000, frame_length_ms 25, frame_shift_ms 10, n_fft 512, n_mels 80, low_freq 20, high_freq 0 (<= 0: from the
  Nyquist frequency), preemph 0.97, delta_order 0 | 1 | 2,
  cmvn      "none" | "utterance" | the path of an .npz with `mean` and `istd` (or `std`) vectors of n_mels entries
  specaug   {n_freq_masks, max_freq_width, n_time_masks, max_time_width}; absent: no masks
  speed_perturb  a list of speed factors chosen uniformly per utterance and epoch, e.g. [0.9, 1.0, 1.1] (Kaldi's three-way
            perturbation; factor s plays round(s sample_rate) samples per second at sample_rate, as sox `speed` does); absent
            or empty: off, and every launch sequence is the one without this key
  reverb    {bank: PATH.npz (or a dict with the same arrays), prob: 0.5, max_taps: 4096}: with probability `prob` an utterance
            is convolved with a room impulse response drawn uniformly from the bank, undelayed and at unit RIR energy
  noise     {bank: PATH.npz (or a dict), prob: 0.5, snr_db: [5, 20]}: with probability `prob` a clip of the bank is added,
            read cyclically from a drawn start, at an SNR drawn uniformly from `snr_db`
            A bank holds `samples` (1-D int16 / float32) and `offsets` (int64 [n + 1]).  Both keys absent by default; then
            every launch sequence is the one without them.

Reverberation and additive noise (csrc/augment.hip; training feeds only) are two passes between the resampler and
the fbank, each launched only when its key is present and the caller hands in draws (`draw_augment`: one generator per row
in collated order, like `draw_speed`).  Neither changes a sample count, so frame counts, `ilens`, the sort of the batch and
the masks' T_b are those without them.
"""
import numpy as np
import torch

import hip_backend as hb


class Frontend(object):
    def __init__(self, cfg=None):
        cfg = dict(cfg or {})
        sr = int(cfg.get("sample_rate", 16000))
        self.plan = hb.FbankPlan(sample_rate=sr,
                                 frame_length=int(round(sr * float(cfg.get("frame_length_ms", 25.0)) / 1000.0)),
                                 frame_shift=int(round(sr * float(cfg.get("frame_shift_ms", 10.0)) / 1000.0)),
                                 n_fft=int(cfg.get("n_fft", 512)), n_mels=int(cfg.get("n_mels", 80)),
                                 low_freq=float(cfg.get("low_freq", 20.0)), high_freq=float(cfg.get("high_freq", 0.0)),
                                 preemph=float(cfg.get("preemph", 0.97)))
        self.n_mels = self.plan.n_mels
        self.delta_order = int(cfg.get("delta_order", 0))
        if self.delta_order not in (0, 1, 2):
            raise hb.UnsupportedShape("frontend: delta_order %d (0, 1 or 2)" % self.delta_order)
        cmvn = cfg.get("cmvn", "none") or "none"
        self._global = None                                    # host [2, n_mels]: mean, istd
        self._global_dev = {}
        if cmvn == "none":
            self.cmvn = hb.CMVN_NONE
        elif cmvn == "utterance":
            self.cmvn = hb.CMVN_UTTERANCE
        else:
            self.cmvn = hb.CMVN_GLOBAL
            with np.load(cmvn) as z:
                mean = np.asarray(z["mean"], dtype=np.float64).reshape(-1)
                istd = (np.asarray(z["istd"], dtype=np.float64) if "istd" in z.files
                        else 1.0 / np.asarray(z["std"], dtype=np.float64)).reshape(-1)
            if mean.size != self.n_mels or istd.size != self.n_mels:
                raise ValueError("frontend: %s holds %d / %d entries for %d mel bins" % (cmvn, mean.size, istd.size, self.n_mels))
            self._global = np.stack([mean, istd]).astype(np.float32)
        sa = dict(cfg.get("specaug") or {})
        self.n_freq_masks, self.max_freq_width = int(sa.get("n_freq_masks", 0)), int(sa.get("max_freq_width", 0))
        self.n_time_masks, self.max_time_width = int(sa.get("n_time_masks", 0)), int(sa.get("max_time_width", 0))
        if not 0 <= self.max_freq_width <= self.n_mels or self.max_time_width < 0 or min(self.n_freq_masks, self.n_time_masks) < 0:
            raise ValueError("frontend: specaug widths and counts must be >= 0, max_freq_width <= n_mels")
        self.speed_factors = [float(s) for s in (cfg.get("speed_perturb") or [])]
        self.resample_plan = hb.ResamplePlan(sr, self.speed_factors) if self.speed_factors else None
        rv, nz = cfg.get("reverb"), cfg.get("noise")
        self.reverb_plan = self.noise_bank = None
        self.reverb_prob = self.noise_prob = 0.0
        self.snr_db = (0.0, 0.0)
        if rv:
            self.reverb_plan = hb.ReverbPlan(hb.load_bank(rv["bank"]), max_taps=int(rv.get("max_taps", 4096)))
            self.reverb_prob = float(rv.get("prob", 0.5))
        if nz:
            self.noise_bank = hb.NoiseBank(hb.load_bank(nz["bank"]))
            self.noise_prob = float(nz.get("prob", 0.5))
            lo, hi = nz.get("snr_db", (5.0, 20.0))
            self.snr_db = (float(lo), float(hi))
            if self.snr_db[0] > self.snr_db[1]:
                raise ValueError("frontend: noise snr_db must be [low, high], got %s" % (self.snr_db,))
        if not (0.0 <= self.reverb_prob <= 1.0 and 0.0 <= self.noise_prob <= 1.0):
            raise ValueError("frontend: reverb / noise `prob` must lie in [0, 1]")

    # ------------------------------------------------------------------ host arithmetic
    @property
    def output_dim(self):
        return self.n_mels * (1 + self.delta_order)

    @property
    def n_masks(self):
        return self.n_freq_masks + self.n_time_masks

    def num_frames(self, n_samples):
        return self.plan.num_frames(n_samples)

    def frames_of(self, waveform):
        """The length filter's and the bucket sort's view of an utterance (dataset.DictDataset(frames_of=...)): the
        UNPERTURBED frame count, also with `speed_perturb` - they see the corpus, not an epoch's draw."""
        return self.num_frames(waveform.shape[0])

    @property
    def n_speeds(self):
        return len(self.speed_factors)

    def draw_speed(self, seed, batch_index, row):
        """The speed factor of one utterance -> its index into `speed_perturb`, uniform.  One numpy generator per row of a
        batch IN COLLATED ORDER (before the feed sorts by perturbed length: the sort depends on the draw, so the draw must
        not depend on the sort), seeded from (seed, batch, row) like draw_masks."""
        rs = np.random.RandomState([int(seed), int(batch_index), int(row)])
        return int(rs.randint(0, self.n_speeds))

    def perturbed_samples(self, n_samples, factor_index):
        """The sample count of an utterance of n_samples after factor `factor_index`: ceil(new n / orig), integers;
        num_frames of it is the perturbed frame count."""
        return self.resample_plan.out_samples(n_samples, factor_index)

    @property
    def augments(self):
        """True with a `reverb` or a `noise` key."""
        return self.reverb_plan is not None or self.noise_bank is not None

    def draw_augment(self, seed, batch_index, row):
        """The reverberation and noise of one utterance -> (RIR index or -1, clip index or -1, noise start, snr_db).  One numpy
        generator per row of a batch IN COLLATED ORDER, seeded from (seed, batch, row) like draw_speed.  Six uniform variates
        in a fixed order - RIR Bernoulli, RIR index, noise Bernoulli, clip index, start in [0, len(clip)), snr_db in [lo, hi] -
        every one taken whether or not it is used (also without its key), so no field's value depends on another's outcome."""
        rs = np.random.RandomState([int(seed), int(batch_index), int(row)])
        u = rs.random_sample(6)
        n_rirs = len(self.reverb_plan) if self.reverb_plan is not None else 0
        n_clips = len(self.noise_bank) if self.noise_bank is not None else 0
        rir = min(int(u[1] * n_rirs), n_rirs - 1) if n_rirs and u[0] < self.reverb_prob else -1
        clip = min(int(u[3] * n_clips), n_clips - 1) if n_clips else -1
        start = 0
        if n_clips:
            n = self.noise_bank.clip_len(clip)
            start = min(int(u[4] * n), n - 1)
        if not u[2] < self.noise_prob:
            clip = -1
        snr_db = self.snr_db[0] + (self.snr_db[1] - self.snr_db[0]) * float(u[5])
        return rir, clip, start, snr_db

    @staticmethod
    def snr_scale(snr_db):
        """10^(-snr_db / 20) as the float32 the device multiplies by: there is no pow on the device."""
        return np.float32(10.0 ** (-float(snr_db) / 20.0))

    def draw_masks(self, seed, batch_index, global_row, T_b):
        """The SpecAugment masks of one utterance: int32 [n_masks, 2] of (start, width), frequency masks first.  One numpy
        generator per GLOBAL row of a batch, seeded from (seed, batch, row) - feed.py's scheme for its input noise: a rank
        draws its own rows only and the union of the rank-local batches is the one-process batch.  Widths are uniform in
        [0, max width] (time: at most T_b), starts uniform over the positions that keep the mask inside."""
        rs = np.random.RandomState([int(seed), int(batch_index), int(global_row)])
        out = np.zeros((self.n_masks, 2), dtype=np.int32)
        for m in range(self.n_freq_masks):
            w = int(rs.randint(0, self.max_freq_width + 1))
            out[m] = (int(rs.randint(0, self.n_mels - w + 1)), w)
        for m in range(self.n_freq_masks, self.n_masks):
            w = int(rs.randint(0, min(self.max_time_width, int(T_b)) + 1))
            out[m] = (int(rs.randint(0, max(int(T_b) - w, 0) + 1)), w)
        return out

    # ------------------------------------------------------------------ device
    def _stats_global(self, device):
        key = str(device)
        t = self._global_dev.get(key)
        if t is None:
            t = self._global_dev[key] = torch.from_numpy(self._global).to(device)
        return t

    def run(self, samples, offsets, frame_lens, t_max, masks=None, speed=None, augment=None):
        """Device tensors in (packed samples int16 / float32, offsets int64 [B + 1], frame_lens int32 [B] = num_frames of
        every sample count, masks int32 [B, n_masks, 2] or None), launches on the current stream -> xs [B, t_max, D].
        speed: None, or (factor_index int32 [B], out_offsets int64 [B + 1] on the device, the host integers out_offsets[B]
        and the longest perturbed sample count): the resample launch runs first, the fbank reads its float32 output, and
        frame_lens are the PERTURBED frame counts.
        augment: None, or (rir_index int32 [B], clip_index int32 [B], start int64 [B], scale float32 [B] on the device, the
        host integers offsets[B] and the longest sample count - perturbed ones with `speed`): reverb, then noise mix, run
        between the resampler and the fbank, each only with its key; every sample and frame count stays."""
        B = offsets.numel() - 1
        dev = samples.device
        ours = False                                           # `samples` is a buffer made here: the mix may run in place
        if speed is not None:
            factor_index, out_offsets, total, longest = speed
            resampled = torch.empty(int(total), device=dev, dtype=torch.float32)
            samples = hb.resample(self.resample_plan, samples, offsets, factor_index, out_offsets, resampled, max_out=int(longest))
            offsets, ours = out_offsets, True
        if augment is not None:
            rir_index, clip_index, start, scale, total, longest = augment
            if self.reverb_plan is not None:
                wet = torch.empty(int(total), device=dev, dtype=torch.float32)
                samples = hb.reverb(self.reverb_plan, samples, offsets, rir_index, wet, max_len=int(longest))
                ours = True
            if self.noise_bank is not None:
                mixed = samples if ours else torch.empty(int(total), device=dev, dtype=torch.float32)
                samples = hb.noise_mix(self.noise_bank, samples, offsets, clip_index, start, scale, out=mixed,
                                       max_len=int(longest))
        static = torch.empty(B, int(t_max), self.n_mels, device=dev, dtype=torch.float32)
        hb.fbank(self.plan, samples, offsets, int(t_max), static, use_log=True)
        stats = None
        if self.cmvn == hb.CMVN_UTTERANCE:
            stats = hb.feat_cmvn_stats(static, self.n_mels, frame_lens,
                                       torch.empty(B, 2, self.n_mels, device=dev, dtype=torch.float32))
        elif self.cmvn == hb.CMVN_GLOBAL:
            stats = self._stats_global(dev)
        out = torch.empty(B, int(t_max), self.output_dim, device=dev, dtype=torch.float32)
        with_masks = masks is not None and self.n_masks > 0
        return hb.feat_finish(static, self.n_mels, frame_lens, out, order=self.delta_order, cmvn=self.cmvn, stats=stats,
                              masks=masks if with_masks else None, n_freq_masks=self.n_freq_masks if with_masks else 0,
                              n_time_masks=self.n_time_masks if with_masks else 0)

    def __call__(self, samples, offsets, masks=None, t_max=None, factor_index=None, augment=None):
        """samples: ONE packed 1-D int16 / float32 tensor on the GPU; offsets: B + 1 host integers; masks: host int32
        [B, n_masks, 2] or None; factor_index: B host indices into `speed_perturb` or None -> (xs [B, T_max, D], ilens: host
        list; with factor_index the perturbed frame counts).  augment: None or B host tuples (RIR index or -1, clip index or
        -1, noise start, snr_db) as `draw_augment` returns them; `samples` itself is never written."""
        if not samples.is_cuda:
            raise RuntimeError("Frontend: samples must live on the GPU: the HIP path has no CPU fallback")
        offs = [int(o) for o in offsets]
        counts = [b - a for a, b in zip(offs[:-1], offs[1:])]
        speed = None
        if factor_index is not None:
            if self.resample_plan is None:
                raise ValueError("Frontend: factor indices need the `speed_perturb` key")
            fi = [int(f) for f in factor_index]
            if len(fi) != len(counts) or min(fi) < 0 or max(fi) >= self.n_speeds:
                raise hb.UnsupportedShape("Frontend: factor indices %s for %d rows, %d factors" % (fi, len(counts), self.n_speeds))
            counts = [self.perturbed_samples(n, f) for n, f in zip(counts, fi)]
            out_offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        ilens = [self.num_frames(n) for n in counts]
        t_max = max(ilens) if t_max is None else int(t_max)
        if t_max < 1:
            raise ValueError("Frontend: no utterance of the batch has a whole frame (%d samples)" % self.plan.frame_length)
        dev = samples.device
        masks_d = hb.to_device_i32(np.asarray(masks, dtype=np.int32), dev) if masks is not None and self.n_masks else None
        if factor_index is not None:
            speed = (hb.to_device_i32(fi, dev), hb.to_device_i64(out_offs, dev), int(out_offs[-1]), max(counts))
        aug = None
        if augment is not None:
            if not self.augments:
                raise ValueError("Frontend: augment draws need the `reverb` or the `noise` key")
            draws = [tuple(a) for a in augment]
            n_rirs = len(self.reverb_plan) if self.reverb_plan is not None else 0
            n_clips = len(self.noise_bank) if self.noise_bank is not None else 0
            if len(draws) != len(counts) or any(not -1 <= int(a[0]) < n_rirs or not -1 <= int(a[1]) < n_clips for a in draws):
                raise hb.UnsupportedShape("Frontend: augment draws %s for %d rows, %d RIRs, %d clips"
                                          % (draws, len(counts), n_rirs, n_clips))
            aug = (hb.to_device_i32([int(a[0]) for a in draws], dev), hb.to_device_i32([int(a[1]) for a in draws], dev),
                   hb.to_device_i64([int(a[2]) for a in draws], dev),
                   hb.to_device_f32(np.asarray([self.snr_scale(a[3]) for a in draws], dtype=np.float32), dev),
                   sum(counts), max(counts))
        xs = self.run(samples, hb.to_device_i64(offs, dev), hb.to_device_i32(ilens, dev), t_max, masks_d, speed, aug)
        return xs, ilens
