"""kapre_amd -- Kapre's time-frequency hot path on AMD Instinct MI355X (gfx950).

Import surface mirrors /root/reference/kapre/__init__.py for the components in scope
(``import kapre_amd as kapre`` is the intended drop-in): the layers run hand-written HIP kernels
through a C ABI (include/kapre_hip.h); there is no CPU fallback.
"""
__version__ = '0.4.0+mi355x.1'
VERSION = __version__

from . import backend
from . import composed

from .keras_shim import Layer, Sequential, Model, Input, register_keras_serializable

from .time_frequency import (
    STFT,
    InverseSTFT,
    Magnitude,
    Phase,
    MagnitudeToDecibel,
    ApplyFilterbank,
    Delta,
    ConcatenateFrequencyMap,
    PCEN,
    CMVN,
    GriffinLim,
    TimeStretch,
    HPSS,
)

from . import signal
from .signal import Frame, Energy, MuLawEncoding, MuLawDecoding, LogmelToMFCC, Resample, LFilter, Preemphasis, Deemphasis, Convolve, PitchShift

from . import augmentation
from .augmentation import SpecAugment, ChannelSwap, Reverb, AddNoise

from .composed import (
    get_stft_magnitude_layer,
    get_melspectrogram_layer,
    get_log_frequency_spectrogram_layer,
    get_perfectly_reconstructing_stft_istft,
    get_stft_mag_phase,
    get_time_stretch_layer,
    get_hpss_layer,
)



def check_device(device=None):
    """Report what only a kernel can see: waits for ``device`` (default: the current one), then reads
    and clears the library's status word.  Raises ``RuntimeError`` naming the kernels when a bounded in-kernel wait ran out or a
    packed filterbank changed under a cached band plan since the last check -- the outputs of the affected launches are wrong --
    and returns ``None`` otherwise.  ``Sequential.predict`` does this after its copy; callers that hand torch tensors to the
    layers call it once per batch (or less often, if a late error is acceptable): the failed launch itself cannot report, the
    NEXT forward call would."""
    import torch
    from . import _ffi
    if torch.cuda.is_available():
        torch.cuda.synchronize(device)
    _ffi.device_status(synchronize=False, raise_on_error=True)

def install_as_kapre():
    """Make ``import kapre`` mean this package: registers it in ``sys.modules`` as ``kapre`` and its modules as
    ``kapre.backend``, ``kapre.composed``, ``kapre.time_frequency``, ``kapre.signal`` and ``kapre.augmentation``, so that the
    ``from kapre import ...`` / ``from kapre.time_frequency import ...`` lines of an existing model run unedited.  Opt-in: nothing
    happens unless it is called; a second call changes nothing.  Raises ``RuntimeError`` when another ``kapre`` is already
    imported or can be found on the path -- shadowing a real installation silently would be worse than editing an import."""
    import importlib.util
    import sys

    this = sys.modules[__name__]
    have = sys.modules.get('kapre')
    if have is not None and have is not this:
        raise RuntimeError('install_as_kapre: another module named kapre is already imported (%r)' % (have,))
    if have is None and importlib.util.find_spec('kapre') is not None:
        raise RuntimeError('install_as_kapre: a kapre package can be imported from %s; remove it from the path or import '
                           'kapre_amd under its own name' % (importlib.util.find_spec('kapre').origin,))
    sys.modules['kapre'] = this
    for name in ('backend', 'composed', 'time_frequency', 'signal', 'augmentation'):
        sys.modules['kapre.' + name] = sys.modules[__name__ + '.' + name]


__all__ = [
    '__version__',
    'VERSION',
    'check_device',
    'install_as_kapre',
    'STFT',
    'InverseSTFT',
    'Magnitude',
    'Phase',
    'MagnitudeToDecibel',
    'ApplyFilterbank',
    'Delta',
    'ConcatenateFrequencyMap',
    'PCEN',
    'CMVN',
    'GriffinLim',
    'TimeStretch',
    'HPSS',
    'Frame',
    'Energy',
    'MuLawEncoding',
    'MuLawDecoding',
    'LogmelToMFCC',
    'Resample',
    'PitchShift',
    'LFilter',
    'Preemphasis',
    'Deemphasis',
    'Convolve',
    'SpecAugment',
    'ChannelSwap',
    'Reverb',
    'AddNoise',
    'get_stft_magnitude_layer',
    'get_melspectrogram_layer',
    'get_log_frequency_spectrogram_layer',
    'get_perfectly_reconstructing_stft_istft',
    'get_stft_mag_phase',
    'get_time_stretch_layer',
    'get_hpss_layer',
    'Layer',
    'Sequential',
    'Model',
    'Input',
]
