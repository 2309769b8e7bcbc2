"""The slice of the Keras Layer / Sequential protocol that Kapre's layers and tests rely on.

The reference's "operator API" is the Keras layer protocol:
``Layer.__init__(**kwargs)`` swallowing ``name`` / ``input_shape`` / ``dtype``,
``__call__(x, training=None) -> call(x)`` (``call(x, training=...)`` for the layers whose ``call`` takes it), ``get_config()`` / ``from_config()``,
``@register_keras_serializable(package='Kapre')`` and composition in ``keras.Sequential``
(``add``, ``.layers``, ``.name``, ``__call__``, ``predict(np) -> np``, ``get_config``).
TensorFlow/Keras are not available on the target image, so this module re-provides exactly that
protocol in plain Python; tensors are torch tensors (device memory container only).

``Sequential`` additionally performs peephole fusion of Kapre layer chains into single HIP
launches (see kapre_amd.time_frequency.fuse_and_run); ``.layers`` still exposes the individual
layers, which remain individually callable, as the reference documents (composed.py:1-13).

Persistence (round 5; the reference's tests/utils.py:60-112 ``save_load_compare``): ``model.save(path)`` /
``load_model(path, custom_objects=None)`` and static shapes (``compute_output_shape`` / ``output_shape`` /
``input_shape``).  Every layer of the path is parameter free, so a saved model IS its config: ``*.keras`` files are zip
archives laid out as Keras 3 writes them (``config.json`` + ``metadata.json``; no ``model.weights.h5`` member -- there
are no weights and h5py is not on the image), any other extension (``*.h5``, ``*.json``) holds the same JSON as text.
"""
from __future__ import annotations

import collections
import datetime
import inspect
import io
import json
import os
import zipfile
from typing import Any, Dict, List, Optional

import numpy as np

_NAME_COUNTS: Dict[str, int] = collections.defaultdict(int)
_REGISTRY: Dict[str, type] = {}
_TAKES_TRAINING: Dict[type, bool] = {}


def _to_snake_case(name: str) -> str:
    out = []
    for i, ch in enumerate(name):
        if ch.isupper() and i > 0 and (not name[i - 1].isupper() or
                                       (i + 1 < len(name) and name[i + 1].islower())):
            out.append('_')
        out.append(ch.lower())
    return ''.join(out)


def _unique_name(prefix: str) -> str:
    n = _NAME_COUNTS[prefix]
    _NAME_COUNTS[prefix] += 1
    return prefix if n == 0 else '%s_%d' % (prefix, n)


def register_keras_serializable(package: str = 'Custom', name: Optional[str] = None):
    """Same decorator signature as tf.keras.utils.register_keras_serializable."""

    def decorator(cls):
        registered = '%s>%s' % (package, name or cls.__name__)
        cls._keras_registered_name = registered
        _REGISTRY[registered] = cls
        _REGISTRY[cls.__name__] = cls
        return cls

    return decorator


def get_registered_object(name: str):
    return _REGISTRY.get(name)


def _takes_training(cls) -> bool:
    """True when ``cls.call`` has a ``training`` parameter (looked up once per class)."""
    takes = _TAKES_TRAINING.get(cls)
    if takes is None:
        takes = _TAKES_TRAINING[cls] = 'training' in inspect.signature(cls.call).parameters
    return takes


class Layer:
    """Minimal keras.layers.Layer: naming, config round trip, __call__ -> call.

    Contract of the layers defined in THIS package (``fuse_and_run`` relies on it when, in training, it lets ``SpecAugment``
    mask the output of the layer in front of it in place): ``call`` returns either its input object or a tensor that the
    layer does not keep a reference to.  A view of the input is recognised by its storage and treated as the input; a layer
    that caches what it returns must live outside the package's modules or copy.  Layers defined elsewhere are never
    assumed to follow this."""

    def __init__(self, name: Optional[str] = None, input_shape=None, dtype=None,
                 trainable: bool = True, batch_input_shape=None, **kwargs):
        if kwargs:
            raise TypeError('Unrecognized keyword arguments passed to %s: %s'
                            % (type(self).__name__, sorted(kwargs)))
        self.name = name if name is not None else _unique_name(_to_snake_case(type(self).__name__))
        self.trainable = trainable
        self._dtype = dtype or 'float32'
        self._input_shape_arg = tuple(input_shape) if input_shape is not None else None
        if batch_input_shape is not None:
            self._input_shape_arg = tuple(batch_input_shape[1:])

    @property
    def dtype(self):
        return self._dtype

    @property
    def _f64(self) -> bool:
        """Keras casts a layer's inputs to the layer dtype (autocast): a layer built with dtype='float64'
        computes in float64 / complex128, every other layer in float32 / complex64."""
        return str(self._dtype) in ('float64', 'double', "<class 'numpy.float64'>", 'torch.float64')

    @property
    def weights(self):
        return []

    def count_params(self) -> int:
        return 0          # all Kapre hot-path layers are parameter free (docs/quickstart.rst:76-78); PCEN can learn its own

    def parameters(self):
        """the layer's learned ``torch.nn.Parameter`` objects, for a torch optimiser (none but for ``PCEN(trainable_params=...)``)"""
        return []

    def build(self, input_shape):
        pass

    def compute_output_shape(self, input_shape):
        """static shape inference, ``None`` for unknown dimensions (keras.layers.Layer.compute_output_shape)"""
        return tuple(input_shape)

    @property
    def input_shape(self):
        if self._input_shape_arg is None:
            raise AttributeError('The layer "%s" has never been called and thus has no defined input shape.' % self.name)
        return (None,) + tuple(self._input_shape_arg)

    @property
    def output_shape(self):
        return self.compute_output_shape(self.input_shape)

    def call(self, x):
        return x

    def __call__(self, x, training=None, **kwargs):
        # the layers that behave differently in training (augmentation.py, Sequential) declare ``training`` in ``call``
        if training is not None and _takes_training(type(self)):
            return self.call(x, training=training)
        return self.call(x)

    def get_config(self) -> Dict[str, Any]:
        return {'name': self.name, 'trainable': self.trainable, 'dtype': self._dtype}

    @classmethod
    def from_config(cls, config: Dict[str, Any]):
        return cls(**config)


class InputLayer(Layer):
    """keras.Input(shape=...) placeholder: records the per-sample shape, passes data through."""

    def __init__(self, shape=None, dtype=None, name=None, batch_size=None, **kwargs):
        super().__init__(name=name, dtype=dtype)
        self.shape = tuple(shape) if shape is not None else None

    def get_config(self):
        config = super().get_config()
        config.update({'shape': self.shape})
        return config


def Input(shape=None, dtype=None, name=None, batch_size=None, **kwargs):
    return InputLayer(shape=shape, dtype=dtype, name=name, batch_size=batch_size)


class Sequential(Layer):
    """keras.Sequential over Kapre layers, with kernel fusion at call time."""

    def __init__(self, layers: Optional[List[Layer]] = None, name: Optional[str] = None,
                 trainable: bool = True):
        super().__init__(name=name if name is not None else _unique_name('sequential'),
                         trainable=trainable)
        self._layers: List[Layer] = []
        for layer in layers or []:
            self.add(layer)

    @property
    def layers(self) -> List[Layer]:
        return [l for l in self._layers if not isinstance(l, InputLayer)]

    def add(self, layer) -> None:
        if not isinstance(layer, Layer):
            raise TypeError('The added layer must be an instance of class Layer. Received: %r'
                            % (layer,))
        self._layers.append(layer)

    def pop(self):
        return self._layers.pop()

    def _flat_layers(self) -> List[Layer]:
        flat: List[Layer] = []
        for layer in self._layers:
            if isinstance(layer, InputLayer):
                continue
            if isinstance(layer, Sequential):
                flat.extend(layer._flat_layers())
            else:
                flat.append(layer)
        return flat

    def call(self, x, training=None):
        from .time_frequency import fuse_and_run
        return fuse_and_run(self._flat_layers(), x, training=training)

    # -- learned parameters: the layers' own, in the order of the layers --------------------------------
    def parameters(self):
        return [p for layer in self._flat_layers() for p in layer.parameters()]

    @property
    def weights(self):
        return [w for layer in self._flat_layers() for w in layer.weights]

    def count_params(self) -> int:
        return sum(layer.count_params() for layer in self._flat_layers())

    # -- static shapes ------------------------------------------------------------------------------
    @property
    def input_shape(self):
        for layer in self._layers:                                   # keras.Input(shape=...) or the first layer's input_shape=
            if isinstance(layer, InputLayer):
                if layer.shape is not None:
                    return (None,) + tuple(layer.shape)
                continue
            return layer.input_shape
        raise AttributeError('The model "%s" has no layers and thus no defined input shape.' % self.name)

    def compute_output_shape(self, input_shape):
        shape = tuple(input_shape)
        for layer in self._layers:
            if not isinstance(layer, InputLayer):
                shape = layer.compute_output_shape(shape)
        return shape

    # -- persistence (reference tests/utils.py:60-112) --------------------------------------------------
    def save(self, filepath, overwrite=True, save_format=None, **kwargs):
        save_model(self, filepath, overwrite=overwrite)

    def predict(self, x, batch_size=None, verbose=0, **kwargs) -> np.ndarray:
        """numpy in -> numpy out (the way the reference's tests drive models)."""
        import torch

        y = self(x)
        if isinstance(y, torch.Tensor):
            host = y.detach().cpu().numpy()
            if y.is_cuda:
                # the copy waited for the kernels: a kernel that gave up one of its bounded waits has said so by now
                # (include/kapre_hip.h: kpr_device_status) -- wrong values never leave predict() silently
                from . import _ffi
                _ffi.device_status(synchronize=False)
            return host
        return np.asarray(y)

    def get_config(self):
        specs = [{'class_name': type(l).__name__,
                  'registered_name': type(l).__dict__.get('_keras_registered_name'),     # (the class's own registration, not a base's)
                  'config': l.get_config()} for l in self._layers]
        # a first layer built with input_shape=...: Keras records it as an InputLayer in front (the layer's own config does
        # not carry it), so that the loaded model knows its input / output shapes
        if self._layers and not isinstance(self._layers[0], InputLayer) and self._layers[0]._input_shape_arg is not None:
            specs.insert(0, {'class_name': 'InputLayer', 'registered_name': None,
                             'config': {'shape': list(self._layers[0]._input_shape_arg), 'dtype': None, 'name': 'input_layer'}})
        return {'name': self.name, 'layers': specs}

    @classmethod
    def from_config(cls, config, custom_objects=None):
        layers = []
        for spec in config['layers']:
            klass = _resolve_class(spec, custom_objects)
            if klass is Sequential or (isinstance(klass, type) and issubclass(klass, Sequential)):
                layers.append(klass.from_config(spec['config'], custom_objects=custom_objects))
            else:
                layers.append(klass.from_config(spec['config']))
        return cls(layers, name=config.get('name'))

    def summary(self, print_fn=print):
        print_fn('Model: "%s"' % self.name)
        for l in self.layers:
            print_fn('  %-32s %s' % (l.name, type(l).__name__))
        print_fn('Total params: %d' % self.count_params())


Model = Sequential


def _resolve_class(spec, custom_objects=None):
    """class of a serialized layer: ``custom_objects`` first (by class name, as keras.models.load_model does), then the
    ``register_keras_serializable`` registry, then the shim's own classes"""
    name = spec['class_name']
    if custom_objects and name in custom_objects and custom_objects[name] is not None:
        return custom_objects[name]
    klass = get_registered_object(spec.get('registered_name') or '') or get_registered_object(name)
    if klass is None:
        klass = {'InputLayer': InputLayer, 'Sequential': Sequential}.get(name)
    if klass is None:
        raise ValueError('Unknown layer: %r. Please ensure you are using a `custom_objects` argument or that the class is '
                         'decorated with `register_keras_serializable`.' % name)
    return klass


def _serialize(model) -> Dict[str, Any]:
    return {'module': 'keras', 'class_name': type(model).__name__,
            'registered_name': type(model).__dict__.get('_keras_registered_name'), 'config': model.get_config()}


def save_model(model, filepath, overwrite=True):
    """``*.keras``: a zip archive with ``config.json`` and ``metadata.json`` (the layout of Keras 3; no weights member: the
    layers of the path have none); any other extension: the same JSON as text."""
    filepath = os.fspath(filepath)
    if os.path.exists(filepath) and not overwrite:
        raise FileExistsError(filepath)
    if not isinstance(model, Layer):
        raise TypeError('save_model expects a model / layer of this module, got %r' % (model,))
    payload = json.dumps(_serialize(model), indent=1)
    if filepath.endswith('.keras'):
        meta = json.dumps({'keras_version': 'kapre_amd.keras_shim', 'date_saved': datetime.datetime.now().strftime('%Y-%m-%d@%H:%M:%S')})
        buf = io.BytesIO()
        with zipfile.ZipFile(buf, 'w') as z:
            z.writestr('metadata.json', meta)
            z.writestr('config.json', payload)
        with open(filepath, 'wb') as f:
            f.write(buf.getvalue())
    else:
        with open(filepath, 'w') as f:
            f.write(payload)


def load_model(filepath, custom_objects=None, compile=True, **kwargs):
    """keras.models.load_model for files written by ``save_model`` / ``Sequential.save``"""
    filepath = os.fspath(filepath)
    if zipfile.is_zipfile(filepath):
        with zipfile.ZipFile(filepath) as z:
            spec = json.loads(z.read('config.json').decode())
    else:
        with open(filepath) as f:
            spec = json.load(f)
    klass = _resolve_class(spec, custom_objects)
    if isinstance(klass, type) and issubclass(klass, Sequential):
        return klass.from_config(spec['config'], custom_objects=custom_objects)
    return klass.from_config(spec['config'])
