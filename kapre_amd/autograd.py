"""Backward passes of the hot-path layers: Kapre's layers are TensorFlow graphs, so a front end placed
inside ``model.fit`` / ``tf.GradientTape`` is differentiable (reference: time_frequency.py:146-187,
:289-319, :351-359, :402, :535-548; backend.py:186-192).  Here a layer called on a torch tensor that
``requires_grad`` returns a tensor with a ``grad_fn`` whose backward runs on the same HIP library:

* the LINEAR layers are their own adjoints' kernels -- ``STFT^T`` is an inverse-STFT launch
  (window ``n_fft * w``, interior bins halved), ``InverseSTFT^T`` an STFT launch (window
  ``2 / n_fft * w_synth``, edge bins halved), ``ApplyFilterbank^T`` / ``LogmelToMFCC^T`` the same
  GEMM with the transposed matrix; ``Frame`` / ``Energy`` / ``Delta`` have gather-form adjoint kernels;
* ``SpecAugment^T`` is its own out-of-place kernel on the cotangent with the saved mask table and mask value 0,
  ``ChannelSwap^T`` the channel gather with the inverse permutation; ``ConcatenateFrequencyMap^T`` drops the map channel
  of the cotangent (one kernel); mu-law decoding of float codes has an elementwise backward kernel, mu-law encoding
  returns integers and ends the tape; ``PCEN`` keeps its smoother ``S`` (the forward kernel's second output) and runs
  one backward kernel, the forward scan in reversed time (input gradient only: its parameters are constants);
  ``CMVN`` keeps its output and ``rstd`` per column and runs one backward kernel, two sums along time and a sweep;
  ``Resample^T`` is the forward's polyphase kernel with the adjoint table; ``LFilter^T`` is its sections in reverse order,
  each the forward kernel scanning in the other direction; ``Convolve^T`` is the forward's three launches with the filter
  table of the time-reversed impulse responses (which are constants: no gradient reaches them); ``AddNoise`` is not linear
  (its gain follows the item's energy): backward is its two kernels in their other modes, a dot product with the wrapped
  noise and ``gy + coef x``, from the saved input, draw table and stats rows;
* ``Magnitude`` / ``Phase`` / ``MagnitudeToDecibel`` have elementwise backward kernels
  (``csrc/kpr_grad_kernels.h``) that follow TensorFlow's registered gradients, including the part of
  the decibel gradient that reaches an item's maximum through the dynamic-range floor;
* a fused chain (one forward launch) is differentiated by recomputation: backward re-runs the chain
  layer by layer with these functions and differentiates that.

Complex cotangents use the convention torch and TensorFlow share (``dL/dRe + i dL/dIm``).
torch.autograd is the tape; every arithmetic step is a HIP launch of this package.
"""
from __future__ import annotations

import numpy as np

from . import _ffi

_CH_LAST_STR = 'channels_last'

# activations (complex spectrum + magnitudes) ChainFn.backward recomputes at a time; read at call time
CHAIN_RECOMPUTE_BYTES = 256 << 20


def needs_grad(x) -> bool:
    """True when the caller expects the layer output to be differentiable w.r.t. ``x``."""
    try:
        import torch
    except ImportError:         # pragma: no cover
        return False
    return isinstance(x, torch.Tensor) and x.requires_grad and torch.is_grad_enabled()


def prep(x, dtype_name: str):
    """Device / dtype / layout normalisation of a tensor that carries gradient, done with torch ops so that it is
    recorded (the forward-only path does the same through _ffi.as_device outside the tape)."""
    import torch

    _ffi.require_gpu()
    dtype = getattr(torch, dtype_name)
    if not x.is_cuda:
        x = x.to(torch.device('cuda', torch.cuda.current_device()))
    if x.dtype != dtype:
        x = x.to(dtype)
    return x.contiguous()


def refuse(x, rank: int, rank_text: str, f64_error, f64_text: str):
    """The two refusals of a float32-only operation, asked of the input as given, before anything touches a device:
    ``ValueError(rank_text % shape)`` for a rank other than ``rank``, then ``f64_error(f64_text)`` for float64 / complex128."""
    if len(x.shape) != rank:
        raise ValueError(rank_text % (tuple(x.shape),))
    if _ffi.is_f64(x):
        raise f64_error(f64_text)


def to_device(x, dtype_name: str):
    """(tensor, recorded): ``x`` as a contiguous tensor of that dtype on the GPU -- through ``prep`` when the call is to be
    recorded for autograd, else through ``_ffi.as_device`` -- and which of the two it was."""
    import torch

    if needs_grad(x):
        return prep(x, dtype_name), True
    return _ffi.as_device(x, getattr(torch, dtype_name)), False


def intake(x, rank: int, dtype_name: str, rank_text: str, f64_error, f64_text: str):
    """``refuse``, then ``to_device``: the whole intake of an operation that has nothing to do in between."""
    refuse(x, rank, rank_text, f64_error, f64_text)
    return to_device(x, dtype_name)


def _scaled_window(layer, key, device, f64: bool, scale: float):
    """``scale * layer.window_fn(win_length)`` on the device, cached on the layer."""
    from . import backend

    def make():
        w = backend.window_values(layer.window_fn, int(layer.win_length), np.float64)
        return (w * scale).astype(np.float64 if f64 else np.float32)

    return layer._consts.get((key, f64, int(layer.win_length), int(layer.n_fft), id(layer.window_fn)), device, make)


# ---------------------------------------------------------------------------------------------
# STFT
# ---------------------------------------------------------------------------------------------
def stft_vjp(layer, gspec, x_shape):
    """Cotangent of the waveform from the cotangent of ``STFT.call``'s complex output.

    X[f, k] = sum_n w[n] x[f hop + n - pad_left] e^{-2 pi i k n / N}, k = 0 .. N/2, so
    dL/dx[t] = sum_f w[n] (Re G[f,0] + (-1)^n Re G[f,N/2] + sum_{0<k<N/2} Re(G[f,k] e^{+2 pi i k n / N})), n = t + pad_left - f hop:
    N * irfft of (G with the interior bins halved), windowed by w and overlap-added -- one inverse-STFT launch."""
    import torch

    n_fft, win, hop = int(layer.n_fft), int(layer.win_length), int(layer.hop_length)
    f64 = gspec.dtype == torch.complex128
    gspec = gspec.contiguous()
    half = _ffi.edge_scale(gspec, n_fft, layer.output_data_format, 1.0, 0.5)
    window = _scaled_window(layer, 'vjp_window', gspec.device, f64, float(n_fft))
    ola = _ffi.istft(half, window, n_fft, win, hop, layer.input_data_format, layer.output_data_format)
    gx = torch.zeros(x_shape, dtype=ola.dtype, device=ola.device)
    pad_left = n_fft - hop if layer.pad_begin else 0
    t_axis = 1 if layer.input_data_format == _CH_LAST_STR else 2
    t_in, t_ola = x_shape[t_axis], ola.shape[t_axis]
    n = min(t_in, t_ola - pad_left)
    if n > 0:
        gx.narrow(t_axis, 0, n).copy_(ola.narrow(t_axis, pad_left, n))
    return gx


def istft_vjp(layer, gwave, n_frames):
    """Cotangent of the (n_fft/2+1)-bin spectrogram from the cotangent of ``InverseSTFT.call``'s waveform.

    y = overlap-add of w_s[n] irfft(X[f])[n]; irfft reads Re / Im of the interior bins with weight 2/N and the real
    parts of DC / Nyquist with weight 1/N, so G[f] = rfft(w_s * gy[f hop : f hop + win]) * (2/N, edges 1/N):
    one STFT launch with window 2 w_s / N, then the edge bins halved."""
    n_fft, win, hop = int(layer.n_fft), int(layer.win_length), int(layer.hop_length)
    import torch

    f64 = gwave.dtype == torch.float64
    gwave = gwave.contiguous()
    window = _scaled_window(layer, 'vjp_window', gwave.device, f64, 2.0 / n_fft)
    b, c, t = _ffi.dims_of(gwave.shape, layer.output_data_format)
    g = _ffi.StftGeom(b, c, t, n_fft, win, hop, 0, 0, _ffi.layout(layer.output_data_format),
                      _ffi.layout(layer.input_data_format))
    f = _ffi.num_frames(g)
    if f != n_frames:     # cannot happen: (F - 1) hop + win samples frame into exactly F frames
        raise RuntimeError('InverseSTFT backward: %d frames, expected %d' % (f, n_frames))
    spec = _ffi.stft(gwave, g, f, window, _ffi.OUT_COMPLEX)
    return _ffi.edge_scale(spec, n_fft, layer.input_data_format, 0.5, 1.0, out=spec)


def _functions():
    """The torch.autograd.Function classes (built on first use: torch is imported lazily everywhere in this package)."""
    global _FN
    if _FN is not None:
        return _FN
    import torch
    from torch.autograd.function import once_differentiable

    class STFTFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, layer):
            ctx.layer, ctx.x_shape = layer, tuple(x.shape)
            return layer._run(x.detach(), _ffi.OUT_COMPLEX)

        @staticmethod
        def backward(ctx, g):
            return stft_vjp(ctx.layer, g, ctx.x_shape), None

    class ISTFTFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, layer):
            ctx.layer, ctx.x_shape = layer, tuple(x.shape)
            return layer._forward(x.detach())

        @staticmethod
        def backward(ctx, g):
            layer, shape = ctx.layer, ctx.x_shape
            ch_last = layer.input_data_format == _CH_LAST_STR
            f_axis, k_axis = (1, 2) if ch_last else (2, 3)
            gs = istft_vjp(layer, g, shape[f_axis])
            k_have, k_in = gs.shape[k_axis], shape[k_axis]
            if k_in > k_have:        # the forward cropped the frequency axis: the cropped bins get no gradient
                full = torch.zeros(shape, dtype=gs.dtype, device=gs.device)
                full.narrow(k_axis, 0, k_have).copy_(gs)
                gs = full
            elif k_in < k_have:      # the forward zero-padded it
                gs = gs.narrow(k_axis, 0, k_in).contiguous()
            return gs, None

    class CplxToRealFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, layer, phase):
            ctx.phase = phase
            y = layer._forward(x.detach())
            # the forward may have cast its input (complex128 -> layer precision never happens; numpy never gets here)
            ctx.save_for_backward(x.detach())
            return y

        @staticmethod
        def backward(ctx, g):
            (x,) = ctx.saved_tensors
            return _ffi.cplx_to_real_bwd(x.contiguous(), g, ctx.phase), None, None

    class MatrixFn(torch.autograd.Function):
        """y = x . M over the frequency axis (ApplyFilterbank, LogmelToMFCC); backward = the same GEMM with M^T."""

        @staticmethod
        def forward(ctx, x, layer, matrix_t, data_format):
            ctx.matrix_t, ctx.data_format = matrix_t, data_format
            return layer._forward(x.detach())

        @staticmethod
        def backward(ctx, g):
            mt = ctx.matrix_t                         # (n_out, n_in) on the device, dtype of the layer
            return _ffi.freq_matmul(g.contiguous().to(mt.dtype), ctx.data_format, mt), None, None, None

    class DbFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, layer):
            ctx.params = (float(layer.ref_value), float(layer.amin), float(layer.dynamic_range))
            y = layer._forward(x.detach())
            ctx.save_for_backward(x.detach().to(y.dtype).contiguous())
            return y

        @staticmethod
        def backward(ctx, g):
            (x,) = ctx.saved_tensors
            return _ffi.mag_to_db_bwd(x, g, *ctx.params), None

    class ChainFn(torch.autograd.Function):
        """A fused run of layers (one forward launch); backward recomputes the chain layer by layer with the
        differentiable functions above and differentiates that (activation recomputation)."""

        @staticmethod
        def forward(ctx, x, layers, run_fused):
            ctx.layers = layers
            ctx.save_for_backward(x.detach())
            return run_fused(layers, x.detach())

        @staticmethod
        @once_differentiable
        def backward(ctx, g):
            """Recomputation is chunked over the batch (every layer of the path treats batch items independently -- the
            decibel maximum is per item, backend.py:178-192): the unfused chain materialises the complex spectrogram and
            the magnitudes, several GB at once for a long batch, ~256 MB per chunk here.  Not differentiable
            a second time (the chain's backward passes are forward launches, not autograd graphs).
            A chunk is recomputed at a smaller batch than the forward ran at and may therefore take another kernel of the
            same arithmetic family (launch-size dispatch): values agree to float32 round-off, so a decibel value that sits
            EXACTLY on the clamp or on a tie of the item maximum may fall on the other side in the recomputation; the
            gradient at such boundaries is that of the recomputed values (tests/test_autograd.py pins ties with inputs that
            are exact in every kernel)."""
            (x,) = ctx.saved_tensors
            if x.numel() == 0:                                   # an empty batch has an empty gradient (no launch)
                return torch.zeros_like(x), None, None
            n = x.shape[0] if x.dim() > 0 else 1
            per_item = max(1, x.numel() // max(n, 1)) * x.element_size()
            first = next((l for l in ctx.layers if getattr(l, 'n_fft', None)), None)    # the chain's STFT, wherever it sits
            n_fft, hop = getattr(first, 'n_fft', None), getattr(first, 'hop_length', None)
            if n_fft and hop:                                   # complex spectrum + magnitude of one item
                per_item = per_item * (n_fft // 2 + 1) * 3 // max(1, hop)
            else:
                per_item *= 4
            step = int(max(1, min(n, CHAIN_RECOMPUTE_BYTES // max(1, per_item))))
            gx = torch.empty_like(x)
            for i0 in range(0, max(n, 1), step):
                with torch.enable_grad():
                    xr = x[i0:i0 + step].detach().requires_grad_(True)
                    y = xr
                    for layer in ctx.layers:
                        y = layer(y)
                    (gc,) = torch.autograd.grad(y, xr, g[i0:i0 + step].to(y.dtype))
                gx[i0:i0 + step] = gc
            return gx, None, None

    class FrameFn(torch.autograd.Function):
        """Frame (energy=False) and Energy (energy=True): both are sums over the frames that cover a sample."""

        @staticmethod
        def forward(ctx, x, layer, energy):
            ctx.layer, ctx.energy, ctx.x_shape = layer, energy, tuple(x.shape)
            xd = x.detach()
            if energy:
                ctx.save_for_backward(xd)
            return layer._forward(xd)

        @staticmethod
        def backward(ctx, g):
            layer = ctx.layer
            g = g.contiguous().to(torch.float32)
            args = (layer.data_format, int(layer.frame_length), int(layer.hop_length), layer.pad_end)
            if ctx.energy:
                (x,) = ctx.saved_tensors
                return _ffi.energy_bwd(x, g, *args, layer._scale()), None, None
            return _ffi.frame_bwd(g, ctx.x_shape, *args), None, None

    class DeltaFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, layer):
            ctx.layer = layer
            return layer._forward(x.detach())

        @staticmethod
        def backward(ctx, g):
            layer = ctx.layer
            g = g.contiguous().to(torch.float32)
            return _ffi.delta(g, layer.data_format, int(layer.win_length), layer.mode, backward=True), None

    class SpecAugmentFn(torch.autograd.Function):
        """y = x off the masks, mask_value on them: the adjoint is the same selection of the cotangent with 0 on the masks
        (the out-of-place apply with the table the forward drew)."""

        @staticmethod
        def forward(ctx, x, layer):
            ctx.layer = layer
            y = layer._forward(x.detach())
            ctx.table = layer.last_mask_table
            return y

        @staticmethod
        def backward(ctx, g):
            return ctx.layer._apply(g.contiguous().to(torch.float32), ctx.table, 0.0), None

    class ChannelGatherFn(torch.autograd.Function):
        """y[c] = x[perm[c]]; backward = the gather with the inverse permutation."""

        @staticmethod
        def forward(ctx, x, ch_axis, perm):
            ctx.ch_axis, ctx.inverse, ctx.dtype = ch_axis, np.argsort(perm).tolist(), x.dtype
            return _ffi.channel_gather(x.detach(), ch_axis, perm)

        @staticmethod
        def backward(ctx, g):
            return _ffi.channel_gather(g.contiguous().to(ctx.dtype), ctx.ch_axis, ctx.inverse), None, None

    class MuLawDecodeFn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, code, quantization_channels):
            ctx.q = quantization_channels
            code = code.detach()
            ctx.save_for_backward(code)
            return _ffi.mu_law_decode(code, quantization_channels)

        @staticmethod
        def backward(ctx, g):
            (code,) = ctx.saved_tensors
            return _ffi.mu_law_decode_bwd(code, g, ctx.q), None

    class FreqMapFn(torch.autograd.Function):
        """y = x with the frequency map as one more channel; backward = the cotangent without that channel."""

        @staticmethod
        def forward(ctx, x, data_format):
            ctx.data_format = data_format
            return _ffi.freq_map_concat(x.detach(), data_format)

        @staticmethod
        def backward(ctx, g):
            return _ffi.freq_map_concat(g.contiguous().to(torch.float32), ctx.data_format, backward=True), None

    class PcenFn(torch.autograd.Function):
        """``s``, ``alpha``, ``delta``, ``r``: device float32 vectors of one value per band, inputs of the Function.  None of
        them needs a gradient: the input-only backward launch.  Any does: kpr_pcen_bwd_params_f32, without the input gradient
        when ``x`` needs none."""

        @staticmethod
        def forward(ctx, x, data_format, s, alpha, delta, r, eps):
            ctx.data_format, ctx.eps = data_format, eps
            x = x.detach()
            params = tuple(None if p is None else p.detach() for p in (s, alpha, delta, r))
            y, smooth = _ffi.pcen(x, data_format, params, eps, want_smooth=True)
            ctx.save_for_backward(x, smooth, *params)
            return y

        @staticmethod
        def backward(ctx, g):
            x, smooth, *params = ctx.saved_tensors
            need = ctx.needs_input_grad
            if not any(need[2:6]):
                return (_ffi.pcen_bwd(x, smooth, g, ctx.data_format, params, ctx.eps),) + (None,) * 6
            gx, gp = _ffi.pcen_bwd_params(x, smooth, g, ctx.data_format, params, ctx.eps, want_gx=need[0])
            return (gx, None) + tuple(gp[i] if need[2 + i] else None for i in range(4)) + (None,)

    class CmvnFn(torch.autograd.Function):
        """y = (x - mean) rstd along time.  The forward launch leaves rstd per column; backward is one launch over the saved
        output y, the cotangent and rstd (without ``norm_vars``: over the cotangent alone, nothing is saved)."""

        @staticmethod
        def forward(ctx, x, data_format, norm_vars, eps):
            ctx.data_format, ctx.norm_vars = data_format, norm_vars
            x = x.detach()
            if not norm_vars:
                return _ffi.cmvn(x, data_format, False, eps)
            y, rstd = _ffi.cmvn(x, data_format, True, eps, want_rstd=True)
            ctx.save_for_backward(y, rstd)
            return y

        @staticmethod
        def backward(ctx, g):
            y, rstd = ctx.saved_tensors if ctx.norm_vars else (None, None)
            return _ffi.cmvn_bwd(y, rstd, g, ctx.data_format, ctx.norm_vars), None, None, None

    class ResampleFn(torch.autograd.Function):
        """y = R x, a linear map: backward = the same polyphase kernel with the adjoint table (one launch)."""

        @staticmethod
        def forward(ctx, x, data_format, forward_plan, adjoint_plan, out_len):
            ctx.data_format, ctx.adjoint_plan = data_format, adjoint_plan
            ctx.in_len = _ffi.dims_of(x.shape, data_format)[2]
            return _ffi.resample(x.detach(), data_format, forward_plan, out_len)

        @staticmethod
        def backward(ctx, g):
            g = g.contiguous().to(torch.float32)
            return _ffi.resample(g, ctx.data_format, ctx.adjoint_plan, ctx.in_len), None, None, None, None

    class ResampleDirectFn(torch.autograd.Function):
        """y = R x with the taps computed on the device, ``out_len`` outputs: backward = the same launch with ``adjoint=1``
        and the input's length."""

        @staticmethod
        def forward(ctx, x, data_format, params, out_len):
            ctx.data_format, ctx.params = data_format, params
            ctx.in_len = _ffi.dims_of(x.shape, data_format)[2]
            return _ffi.resample_direct(x.detach(), data_format, params, False, out_len)

        @staticmethod
        def backward(ctx, g):
            g = g.contiguous().to(torch.float32)
            return _ffi.resample_direct(g, ctx.data_format, ctx.params, True, ctx.in_len), None, None, None

    class LFilterFn(torch.autograd.Function):
        """y = F x, a cascade of biquad sections, each a linear map whose adjoint is the same section run in the other
        direction: backward = the sections in reverse order, each one launch sequence of the forward kernel with ``reverse``
        flipped.  ``plan``: a tuple of (coef, reverse) per launch."""

        @staticmethod
        def forward(ctx, x, data_format, plan):
            ctx.data_format, ctx.plan = data_format, plan
            y = x.detach()
            for coef, reverse in plan:
                y = _ffi.lfilter(y, data_format, coef, reverse)
            return y

        @staticmethod
        def backward(ctx, g):
            g = g.contiguous().to(torch.float32)
            for coef, reverse in reversed(ctx.plan):
                g = _ffi.lfilter(g, ctx.data_format, coef, not reverse)
            return g, None, None

    class ConvolveFn(torch.autograd.Function):
        """y = the samples [first, first + n_out) of x * h, a linear map of the waveform: backward = the same three launches
        with the table of the time-reversed impulse responses on the cotangent, zero-extended to the full length where the
        forward trimmed it, read at [len - 1, len - 1 + T).  The impulse responses are constants and get no gradient."""

        @staticmethod
        def forward(ctx, x, data_format, plan, idx, first, n_out):
            from . import backend
            ctx.data_format, ctx.plan, ctx.idx, ctx.first, ctx.n_out = data_format, plan, idx, first, n_out
            ctx.t_axis = 1 if data_format == _CH_LAST_STR else 2
            ctx.t_in = x.shape[ctx.t_axis]
            full = backend._convolve_full(x.detach(), data_format, plan, idx)
            return full.narrow(ctx.t_axis, first, n_out).contiguous()

        @staticmethod
        def backward(ctx, g):
            from . import backend
            g = g.contiguous().to(torch.float32)
            n_full = ctx.t_in + ctx.plan.ir_len - 1
            if ctx.first != 0 or ctx.n_out != n_full:
                shape = list(g.shape)
                shape[ctx.t_axis] = n_full
                gfull = torch.zeros(shape, dtype=torch.float32, device=g.device)
                gfull.narrow(ctx.t_axis, ctx.first, ctx.n_out).copy_(g)
                g = gfull
            back = backend._convolve_full(g, ctx.data_format, ctx.plan, ctx.idx, adjoint=True)
            return back.narrow(ctx.t_axis, ctx.plan.ir_len - 1, ctx.t_in).contiguous(), None, None, None, None, None

    class AddNoiseFn(torch.autograd.Function):
        """y = x + g(x) seg with the gain g proportional to ||x||: backward is exact, gx = gy + (<gy, seg> g / Sx) x -- the
        forward's two kernels in their other modes (the dot product with the wrapped noise; the stream with x as its plain
        second operand).  Saves x, the draw table and the stats rows, nothing else; noise and snr are constants."""

        @staticmethod
        def forward(ctx, x, data_format, bank, lengths, table):
            ctx.data_format, ctx.bank, ctx.lengths = data_format, bank, lengths
            x = x.detach()
            y, stats = _ffi.add_noise(x, data_format, bank, lengths, table)
            ctx.save_for_backward(x, table, stats)
            ctx.mark_non_differentiable(stats)
            return y, stats

        @staticmethod
        def backward(ctx, g, _gstats):
            x, table, stats = ctx.saved_tensors
            gx, _ = _ffi.add_noise_bwd(g, x, ctx.data_format, ctx.bank, ctx.lengths, table, stats)
            return gx, None, None, None, None

    _FN = dict(add_noise=AddNoiseFn, convolve=ConvolveFn, stft=STFTFn, istft=ISTFTFn, c2r=CplxToRealFn, matrix=MatrixFn, db=DbFn, chain=ChainFn,
               frame=FrameFn, delta=DeltaFn, spec_augment=SpecAugmentFn, channel_gather=ChannelGatherFn,
               mu_law_decode=MuLawDecodeFn, freq_map=FreqMapFn, pcen=PcenFn, cmvn=CmvnFn, resample=ResampleFn, lfilter=LFilterFn,
               resample_direct=ResampleDirectFn)
    return _FN


_FN = None


def stft(layer, x):
    return _functions()['stft'].apply(x, layer)


def istft(layer, x):
    return _functions()['istft'].apply(x, layer)


def magnitude(layer, x):
    return _functions()['c2r'].apply(x, layer, 0)


def phase(layer, x):
    return _functions()['c2r'].apply(x, layer, 1)


def matrix(layer, x, matrix_t, data_format):
    return _functions()['matrix'].apply(x, layer, matrix_t, data_format)


def decibel(layer, x):
    return _functions()['db'].apply(x, layer)


def chain(layers, x, run_fused):
    return _functions()['chain'].apply(x, tuple(layers), run_fused)


def frame(layer, x):
    return _functions()['frame'].apply(x, layer, False)


def energy(layer, x):
    return _functions()['frame'].apply(x, layer, True)


def delta(layer, x):
    return _functions()['delta'].apply(x, layer)


def spec_augment(layer, x):
    return _functions()['spec_augment'].apply(x, layer)


def channel_gather(x, ch_axis, perm):
    return _functions()['channel_gather'].apply(x, ch_axis, perm)


def mu_law_decode(code, quantization_channels):
    return _functions()['mu_law_decode'].apply(code, quantization_channels)


def freq_map_concat(x, data_format):
    return _functions()['freq_map'].apply(x, data_format)


def pcen(x, data_format, params, eps):
    return _functions()['pcen'].apply(x, data_format, *params, eps)


def cmvn(x, data_format, norm_vars, eps):
    return _functions()['cmvn'].apply(x, data_format, norm_vars, eps)


def resample(x, data_format, forward_plan, adjoint_plan, out_len):
    return _functions()['resample'].apply(x, data_format, forward_plan, adjoint_plan, out_len)


def resample_direct(x, data_format, params, out_len):
    return _functions()['resample_direct'].apply(x, data_format, params, out_len)


def lfilter(x, data_format, plan):
    return _functions()['lfilter'].apply(x, data_format, tuple(plan))


def convolve(x, data_format, plan, idx, first, n_out):
    return _functions()['convolve'].apply(x, data_format, plan, idx, first, n_out)


def add_noise(x, data_format, bank, lengths, table):
    """(y, stats) of _ffi.add_noise with y on the tape"""
    return _functions()['add_noise'].apply(x, data_format, bank, lengths, table)
