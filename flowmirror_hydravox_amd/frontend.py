"""Prompt-feature extraction on the device: the three spectral features the zero-shot frontend computes from the prompt
audio (cosyvoice/cli/frontend.py:92-122) — HvxMelSpectrogram (prompt log-mel for the flow, below), HvxWhisperLogMel (128-bin input of the
speech tokenizer, :95) and HvxKaldiFbank (80-bin input of the CAM++ speaker encoder with its mean subtraction, :104-108).  The ONNX
graphs those last two feed are assets of the weights repository and stay outside this build; what runs on the host in the reference —
the feature extraction — runs here as two GEMMs (framing x folded DFT basis, power x mel filterbank) in libhvx: hvx_frame_features.

The log-mel spectrogram the zero-shot frontend computes for the prompt audio — `feat_extractor` = matcha.utils.audio.mel_spectrogram (matcha/utils/audio.py:45-82, called at cosyvoice/cli/frontend.py:119;
CosyVoice3 settings n_fft 1920, hop 480, win 1920, 80 mels, 24 kHz, fmin 0, fmax 8000).  Same call signature as the reference's partial:
    HvxMelSpectrogram(n_fft=1920, num_mels=80, sampling_rate=24000, hop_size=480, win_size=1920, fmin=0, fmax=8000)(y)  ->  (B, num_mels, frames)
STFT and mel projection are fp32-MFMA GEMMs against bases built at construction (libhvx: hvx_mel_spectrogram); no CPU fallback.

In front of them: HvxResample, the band-limited resampler `load_wav` applies to a prompt of any sample rate (cosyvoice/utils/file_utils.py:46-75,
torchaudio.transforms.Resample; libhvx: hvx_op_resample_sinc), and load_wav itself.  Around them: HvxFrontEnd, the reference's `frontend_zero_shot` /
`frontend_sft` (cli/frontend.py:157-184) over these stages — what HvxModelManager's `frontend_factory` returns to serve raw prompts without torchaudio,
whisper or onnxruntime.  The text tokenizer stays the caller's."""
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
import ctypes as C

from .packing import kaldi_fbank_bases, mel_filterbank, sinc_resample_len, sinc_resample_taps, stft_bases, whisper_bases


class HvxMelSpectrogram:
    def __init__(self, n_fft=1920, num_mels=80, sampling_rate=24000, hop_size=480, win_size=1920, fmin=0, fmax=8000, center=False, device='cuda'):
        if center or win_size != n_fft:
            raise NotImplementedError('the reference frontend uses center=False and win_size == n_fft')
        _lib.require_gpu()
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.n_fft, self.hop, self.num_mels = n_fft, hop_size, num_mels
        ana, _, _ = stft_bases(n_fft)
        mel = mel_filterbank(sampling_rate, n_fft, num_mels, fmin, fmax)
        bins = n_fft // 2 + 1
        ld = (bins + 31) // 32 * 32
        melp = torch.zeros(num_mels, ld)
        melp[:, :bins] = mel
        self._ana, self._mel = ana.to(self.device), melp.to(self.device).contiguous()
        self._ws = None

    @torch.inference_mode()
    def __call__(self, y):
        """y: (B, L) float waveform in [-1, 1] -> (B, num_mels, frames)"""
        y = y.to(self.device, torch.float32).contiguous()
        B, L = y.shape
        pad = (self.n_fft - self.hop) // 2
        frames = (L + 2 * pad - self.n_fft) // self.hop + 1
        out = torch.empty(B, self.num_mels, frames, dtype=torch.float32, device=self.device)
        need = self.lib.hvx_mel_workspace_bytes(L, self.n_fft, self.hop, self.num_mels)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        for b in range(B):
            check(self.lib.hvx_mel_spectrogram(stream_ptr(), ptr(self._ws), self._ws.numel(), ptr(y[b]), L, self.n_fft, self.hop, ptr(self._ana),
                                               ptr(self._mel), self.num_mels, ptr(out[b])), 'hvx_mel_spectrogram')
        return out


class _FramedFeatures:
    """shared driver of hvx_frame_features: bases on the device, a growing workspace, one launch chain per waveform"""

    def __init__(self, basis, mel, device):
        _lib.require_gpu()
        self.lib = _lib.load()
        self.device = torch.device(device)
        self._basis, self._mel = basis.to(self.device).contiguous(), mel.to(self.device).contiguous()
        self._ws = None

    def _run(self, y, cfg, out):
        need = self.lib.hvx_frame_features_workspace_bytes(y.numel(), C.byref(cfg))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        check(self.lib.hvx_frame_features(stream_ptr(), ptr(self._ws), self._ws.numel(), ptr(y), y.numel(), C.byref(cfg), ptr(self._basis), ptr(self._mel),
                                          ptr(out)), 'hvx_frame_features')
        return out


class HvxWhisperLogMel(_FramedFeatures):
    """`whisper.log_mel_spectrogram(audio, n_mels=128)` (frontend.py:95; whisper/audio.py:110-157) for 16 kHz audio:
    (L,) or (B, L) -> (n_mels, L // 160) or (B, n_mels, L // 160)"""

    def __init__(self, n_mels=128, device='cuda'):
        basis, mel = whisper_bases(n_mels)
        super().__init__(basis, mel, device)
        self.n_mels = n_mels

    @torch.inference_mode()
    def __call__(self, audio):
        a = audio.to(self.device, torch.float32)
        single = a.dim() == 1
        a = a.reshape(-1, a.shape[-1]).contiguous()
        B, L = a.shape
        if L <= 200:
            raise ValueError('whisper log-mel: the audio must be longer than the 200-sample reflection pad')
        frames = L // 160                                    # 1 + L // 160 STFT frames, the last one dropped (audio.py:149)
        if frames < 1:
            raise ValueError('whisper log-mel: audio shorter than one hop')
        cfg = _lib.FeatureConfig(frame_len=416, hop=160, reflect_pad=200, n_frames=frames, bins=201, power=1, mag_eps=0.0, n_mels=self.n_mels,
                                 log_floor=1e-10, log_scale=0.4342944819032518, post=1, time_major=0)
        out = torch.empty(B, self.n_mels, frames, dtype=torch.float32, device=self.device)
        for b in range(B):                                   # the dynamic-range floor is per call (log_spec.max()): one waveform at a time
            self._run(a[b], cfg, out[b])
        return out[0] if single else out


class HvxKaldiFbank(_FramedFeatures):
    """`kaldi.fbank(speech, num_mel_bins=80, dither=0, sample_frequency=16000)` and the frontend's mean subtraction (frontend.py:104-108):
    (1, L) or (L,) -> (1 + (L - 400) // 160, num_mel_bins)"""

    def __init__(self, num_mel_bins=80, sample_frequency=16000, subtract_mean=True, device='cuda'):
        if int(sample_frequency) != 16000:
            raise NotImplementedError('the reference frontend extracts speaker features at 16 kHz')
        basis, mel = kaldi_fbank_bases(num_mel_bins, float(sample_frequency))
        super().__init__(basis, mel, device)
        self.num_mel_bins, self.subtract_mean = num_mel_bins, subtract_mean

    @torch.inference_mode()
    def __call__(self, waveform):
        a = waveform.to(self.device, torch.float32).reshape(-1).contiguous()
        L = a.numel()
        if L < 400:
            return torch.empty(0, self.num_mel_bins, device=self.device)
        frames = 1 + (L - 400) // 160
        cfg = _lib.FeatureConfig(frame_len=416, hop=160, reflect_pad=0, n_frames=frames, bins=257, power=1, mag_eps=0.0, n_mels=self.num_mel_bins,
                                 log_floor=1.1920928955078125e-07, log_scale=1.0, post=2 if self.subtract_mean else 0, time_major=1)
        return self._run(a, cfg, torch.empty(frames, self.num_mel_bins, dtype=torch.float32, device=self.device))


class HvxSpeechTokenizer:
    """`CosyVoiceFrontEnd._extract_speech_token` on the device (cosyvoice/cli/frontend.py:92-103): 16 kHz prompt audio -> whisper 128-bin log-mel
    (HvxWhisperLogMel) -> the speech-tokenizer ONNX graph through the device executor (onnx_graph.OnnxRunner instead of an onnxruntime CPU session) ->
    (speech_token int32 [1][N], speech_token_len int32 [1]).  The graph's inputs are taken by position, as the reference does
    (`session.get_inputs()[0]` = the features [1][128][T], `[1]` = their length as int32 [1]); a graph with a single input gets the features only.
    `speech_tokenizer_v3.onnx` itself is an asset of the weights repository (not in the tree): parity with onnxruntime on it is unpinned."""

    def __init__(self, onnx_model, device='cuda', allow_uncovered=False):
        from .onnx_graph import OnnxRunner
        self.runner = OnnxRunner(onnx_model, device=device, allow_uncovered=allow_uncovered)          # (refuses a graph outside onnx_graph.COVERED unless told otherwise)
        self.feat = HvxWhisperLogMel(128, device=device)
        self.device = torch.device(device)

    @torch.inference_mode()
    def __call__(self, speech_16k):
        speech = speech_16k.reshape(1, -1)
        if speech.shape[1] / 16000 > 30:
            raise AssertionError('do not support extract speech token for audio longer than 30s')          # (frontend.py:94)
        feat = self.feat(speech)                                                            # [1][128][T]
        names = self.runner.g.inputs
        feeds = {names[0]: feat}                                                            # (stays on the device)
        if len(names) > 1:
            import numpy as np
            feeds[names[1]] = np.array([feat.shape[2]], dtype=np.int32)
        out = self.runner.run(feeds)[self.runner.g.outputs[0]]
        tok = torch.tensor([out.reshape(-1).tolist()], dtype=torch.int32, device=self.device)
        return tok, torch.tensor([tok.shape[1]], dtype=torch.int32, device=self.device)


class HvxSpeakerEncoder:
    """`CosyVoiceFrontEnd._extract_spk_embedding` on the device (cosyvoice/cli/frontend.py:105-115): 16 kHz prompt audio -> kaldi 80-bin fbank with
    mean subtraction (HvxKaldiFbank) -> the CAM++ ONNX graph through the device executor -> embedding float32 [1][D] (D = 192 for campplus.onnx, an
    asset that is not in the tree: parity with onnxruntime on it is unpinned)."""

    def __init__(self, onnx_model, device='cuda', allow_uncovered=False):
        from .onnx_graph import OnnxRunner
        self.runner = OnnxRunner(onnx_model, device=device, allow_uncovered=allow_uncovered)
        self.feat = HvxKaldiFbank(80, 16000, subtract_mean=True, device=device)
        self.device = torch.device(device)

    @torch.inference_mode()
    def __call__(self, speech_16k):
        feat = self.feat(speech_16k.reshape(1, -1))                                         # [frames][80]
        out = self.runner.run({self.runner.g.inputs[0]: feat.unsqueeze(0)})[self.runner.g.outputs[0]]
        return torch.tensor([out.reshape(-1).tolist()], dtype=torch.float32, device=self.device)


class HvxResample:
    """`torchaudio.transforms.Resample(orig_freq, new_freq)` at its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) on the device:
    (L,) or (B, L) float -> (..., ceil(new * L / orig)).  The taps (packing.sinc_resample_taps) are built once and kept on the device; equal rates return
    the input unchanged.  libhvx: hvx_op_resample_sinc (csrc/resample.hip), no CPU fallback."""

    def __init__(self, orig_freq=16000, new_freq=16000, device='cuda'):
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self.device = torch.device(device)
        self._taps = None
        if self.orig_freq != self.new_freq:
            taps, self.width, self.orig, self.new = sinc_resample_taps(self.orig_freq, self.new_freq)      # (refuses a table over 64 MiB before any device work)
            _lib.require_gpu()
            self._taps = taps.t().contiguous().to(self.device)                                            # [K][new]: the phases of a tap contiguous

    @torch.inference_mode()
    def __call__(self, waveform):
        if self._taps is None:
            return waveform
        from .ops import resample_sinc
        x = waveform.to(self.device, torch.float32)
        if x.dim() not in (1, 2):
            raise ValueError('HvxResample takes (L,) or (B, L) waveforms, got %s' % (tuple(x.shape),))
        rows = x.reshape(1, -1) if x.dim() == 1 else x
        if rows.shape[1] > 1 and rows.stride(1) != 1:
            rows = rows.contiguous()
        if rows.numel() == 0:
            y = rows.new_empty(rows.shape[0], sinc_resample_len(0, self.orig, self.new))
        else:
            y = resample_sinc(rows, self._taps, self.orig, self.new, self.width)
        return y[0] if x.dim() == 1 else y


_RESAMPLERS = {}


def load_wav(wav, target_sr, min_sr=16000, device='cuda'):
    """`load_wav` of the reference (cosyvoice/utils/file_utils.py:46-75) for audio that is already decoded: `wav` is (tensor | ndarray, sample_rate) with the
    rate an int, float, numpy scalar or 0-d tensor, or a bare tensor / ndarray taken as already at `target_sr`; channels are averaged to mono, a rate below
    `min_sr` fails the reference's assertion, and the resampling runs on the device (one HvxResample per (orig, new), kept) -> float32 (1, L) on `device`.
    A file path raises NotImplementedError: there is no audio decoder here, the server hands over tensors."""
    import numbers
    import os
    import numpy as np
    sample_rate = None
    if isinstance(wav, (tuple, list)) and len(wav) == 2:
        wav, sample_rate = wav
        if isinstance(sample_rate, torch.Tensor):
            sample_rate = int(sample_rate.item())
        elif isinstance(sample_rate, (np.generic, numbers.Real)):
            sample_rate = int(sample_rate)
    if isinstance(wav, torch.Tensor):
        speech = wav.detach()
    elif isinstance(wav, np.ndarray):
        speech = torch.from_numpy(wav)
    elif isinstance(wav, (str, bytes, os.PathLike)):
        raise NotImplementedError('load_wav: %r is a file path; this package has no audio decoder — pass (tensor, sample_rate)' % (wav,))
    else:
        raise TypeError('load_wav: expected a tensor, an ndarray or (audio, sample_rate), got %s' % type(wav).__name__)
    if speech.dim() == 1:
        speech = speech.unsqueeze(0)
    if not speech.is_floating_point():
        raise TypeError('load_wav: %s audio; the reference decodes to float in [-1, 1]' % speech.dtype)
    if speech.shape[0] > 1:
        speech = speech.mean(dim=0, keepdim=True)
    if sample_rate is None:
        sample_rate = target_sr
    if sample_rate != target_sr:
        assert sample_rate >= min_sr, 'wav sample rate {} must be greater than {}'.format(sample_rate, target_sr)
        key = (int(sample_rate), int(target_sr), str(device))
        if key not in _RESAMPLERS:
            _RESAMPLERS[key] = HvxResample(sample_rate, target_sr, device=device)
        return _RESAMPLERS[key](speech)
    return speech.to(device, torch.float32)


class HvxFrontEnd:
    """The zero-shot / speaker frontend of the reference (`CosyVoiceFrontEnd`, cosyvoice/cli/frontend.py:39-184) composed of this package's device stages,
    for `HvxModelManager(frontend_factory=lambda args, cfg: HvxFrontEnd(...))`: raw prompt audio at any rate -> load_wav (HvxResample) -> HvxSpeechTokenizer,
    HvxSpeakerEncoder and HvxMelSpectrogram, with the `feat = 2 x token` trim (:169-173).  The model inputs carry the reference's keys, dtypes and [1][N]
    shapes (:157-184), on the device.
      tokenize        text -> list[int]: the caller's text tokenizer (the reference's `get_tokenizer().encode`; out of scope here)
      speech_tokenizer_onnx, campplus_onnx   the two ONNX assets (paths or onnx_graph.Graph), run by the device executor
      spk2info        {spk_id: {'embedding': ...}} or the path of a torch-saved one ({} when absent, as the reference)
      text_normalize  (text, split, text_frontend) -> list[str] | str; default: the reference's pass-through for text_frontend=False (no text normaliser here)
    frontend_cross_lingual / frontend_instruct* / frontend_vc are not provided: the HydraVox server never calls them."""

    def __init__(self, tokenize, speech_tokenizer_onnx, campplus_onnx, spk2info=None, text_normalize=None, allow_uncovered=False, device='cuda'):
        import os
        self.tokenize = tokenize
        self.device = torch.device(device)
        self.speech_tokenizer = HvxSpeechTokenizer(speech_tokenizer_onnx, device=device, allow_uncovered=allow_uncovered)
        self.speaker_encoder = HvxSpeakerEncoder(campplus_onnx, device=device, allow_uncovered=allow_uncovered)
        self.feat_extractor = HvxMelSpectrogram(device=device)                                # (the CosyVoice3 settings: 24 kHz, n_fft 1920, hop 480, 80 mels)
        if isinstance(spk2info, (str, os.PathLike)):
            spk2info = torch.load(spk2info, map_location=self.device) if os.path.exists(spk2info) else {}      # (:58-61)
        self.spk2info = {} if spk2info is None else spk2info
        self._text_normalize = text_normalize

    def _extract_text_token(self, text):
        tok = torch.tensor([list(self.tokenize(text))], dtype=torch.int32).reshape(1, -1).to(self.device)
        return tok, torch.tensor([tok.shape[1]], dtype=torch.int32, device=self.device)

    def _extract_speech_token(self, prompt_wav):
        return self.speech_tokenizer(load_wav(prompt_wav, 16000, device=self.device))

    def _extract_spk_embedding(self, prompt_wav):
        return self.speaker_encoder(load_wav(prompt_wav, 16000, device=self.device))

    def _extract_speech_feat(self, prompt_wav):
        feat = self.feat_extractor(load_wav(prompt_wav, 24000, device=self.device)).transpose(1, 2).contiguous()      # [1][frames][80]
        return feat, torch.tensor([feat.shape[1]], dtype=torch.int32, device=self.device)

    def text_normalize(self, text, split=True, text_frontend=True):
        if self._text_normalize is not None:
            return self._text_normalize(text, split=split, text_frontend=text_frontend)
        return [text] if split is True else text

    def frontend_sft(self, tts_text, spk_id):
        text, text_len = self._extract_text_token(tts_text)
        embedding = self.spk2info[spk_id]['embedding']
        return {'text': text, 'text_len': text_len, 'llm_embedding': embedding, 'flow_embedding': embedding}

    def frontend_zero_shot(self, tts_text, prompt_text, prompt_wav, resample_rate, zero_shot_spk_id):
        text, text_len = self._extract_text_token(tts_text)
        if zero_shot_spk_id == '':
            prompt_text_token, prompt_text_len = self._extract_text_token(prompt_text)
            speech_feat, speech_feat_len = self._extract_speech_feat(prompt_wav)
            wav_16k = (load_wav(prompt_wav, 16000, device=self.device), 16000)               # resampled once for the tokenizer and the speaker encoder
            speech_token, speech_token_len = self._extract_speech_token(wav_16k)
            if resample_rate == 24000:
                token_len = min(int(speech_feat.shape[1] / 2), speech_token.shape[1])          # force speech_feat = 2 x speech_token (:169-173)
                # (fresh length tensors, not the reference's in-place writes: the stages return inference-mode tensors)
                speech_feat, speech_feat_len = speech_feat[:, :2 * token_len], torch.tensor([2 * token_len], dtype=torch.int32, device=self.device)
                speech_token, speech_token_len = speech_token[:, :token_len], torch.tensor([token_len], dtype=torch.int32, device=self.device)
            embedding = self._extract_spk_embedding(wav_16k)
            model_input = {'prompt_text': prompt_text_token, 'prompt_text_len': prompt_text_len,
                           'llm_prompt_speech_token': speech_token, 'llm_prompt_speech_token_len': speech_token_len,
                           'flow_prompt_speech_token': speech_token, 'flow_prompt_speech_token_len': speech_token_len,
                           'prompt_speech_feat': speech_feat, 'prompt_speech_feat_len': speech_feat_len,
                           'llm_embedding': embedding, 'flow_embedding': embedding}
        else:
            model_input = dict(self.spk2info[zero_shot_spk_id])                                # (a copy: the stored entry keeps no request's text)
        model_input['text'] = text
        model_input['text_len'] = text_len
        return model_input
