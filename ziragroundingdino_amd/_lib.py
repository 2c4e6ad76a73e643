"""ctypes binding of the C ABI declared in include/zira_msda.h, include/zira_metrics.h, include/zira_rsb_ml.h,
include/zira_nms.h, include/zira_vocab.h, include/zira_lvis.h, include/zira_phrase.h, include/zira_adapter.h, include/zira_clslinear.h, include/zira_prompt.h, include/zira_prompt_memory.h, include/zira_cet.h and include/zira_lora.h, derived from the headers at import (_header.py).

There is deliberately no fallback: if ``libzira_msda.so`` is missing the import of the op
raises, so a GPU box can never silently run a non-HIP path.

Adding an entry point: declare it in the header and implement it in csrc/ -- ``load()`` types it from the declaration.  A new
limit (``#define ZIRA_...``) is in ``CONSTANTS``, a new struct in ``STRUCTS``; give them a name below where Python uses them.
"""
import ctypes
import os

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ZIRA_MSDA_LIB") or os.path.join(_HERE, "libzira_msda.so")  # env: dev A/B builds

_HEADER = os.path.join(_HERE, os.pardir, "include", "zira_msda.h")
_METRICS_HEADER = os.path.join(_HERE, os.pardir, "include", "zira_metrics.h")
_RSB_ML_HEADER = os.path.join(_HERE, os.pardir, "include", "zira_rsb_ml.h")
_NMS_HEADER = os.path.join(_HERE, os.pardir, "include", "zira_nms.h")
_VOCAB_HEADER = os.path.join(_HERE, os.pardir, "include", "zira_vocab.h")
_LVIS_HEADER = os.path.join(_HERE, os.pardir, "include", "zira_lvis.h")
_PHRASE_HEADER = os.path.join(_HERE, os.pardir, "include", "zira_phrase.h")
_ADAPTER_HEADER = os.path.join(_HERE, os.pardir, "include", "zira_adapter.h")
_CLSLINEAR_HEADER = os.path.join(_HERE, os.pardir, "include", "zira_clslinear.h")
_PROMPT_HEADER = os.path.join(_HERE, os.pardir, "include", "zira_prompt.h")
_PMEM_HEADER = os.path.join(_HERE, os.pardir, "include", "zira_prompt_memory.h")
_CET_HEADER = os.path.join(_HERE, os.pardir, "include", "zira_cet.h")
_LORA_HEADER = os.path.join(_HERE, os.pardir, "include", "zira_lora.h")
# Structs whose arrays are rows of a device tensor (optim_tail.py, ema.py): callers pass ``data_ptr()``, a plain address, which
# ``POINTER(struct)`` refuses, so their pointers are ``c_void_p``.  The others are host descriptors built with ctypes.
DEVICE_TABLES = ("zira_optim_segment", "zira_ema_segment", "zira_prompt_segment")


def read_header(path):
    try:
        with open(path) as f:
            return _header.parse(f.read(), DEVICE_TABLES, os.path.basename(path))
    except OSError as e:
        raise _header.HeaderError("cannot read %s (%s): the binding is derived from it" % (path, e)) from e


PROTOTYPES, STRUCTS, CONSTANTS = read_header(_HEADER)
SYMBOLS = tuple(PROTOTYPES)     # every symbol the header declares (tests check the .so exports exactly these)
RowGemmArgs, PlaceImage, ResampleImage = STRUCTS["zira_rowgemm_args"], STRUCTS["zira_place_image"], STRUCTS["zira_resample_image"]
OptimSegment, EmaSegment = STRUCTS["zira_optim_segment"], STRUCTS["zira_ema_segment"]
PLACE_MAX_IMAGES, VOC_MAX_THRS = CONSTANTS["ZIRA_PLACE_MAX_IMAGES"], CONSTANTS["ZIRA_VOC_MAX_THRS"]
AP_MAX_THRS, AP_MAX_AREAS = CONSTANTS["ZIRA_AP_MAX_THRS"], CONSTANTS["ZIRA_AP_MAX_AREAS"]
AP_MAX_DETS, AP_MAX_RECS, AP_MAX_CLASSES = CONSTANTS["ZIRA_AP_MAX_DETS"], CONSTANTS["ZIRA_AP_MAX_RECS"], CONSTANTS["ZIRA_AP_MAX_CLASSES"]
RESAMPLE_MAX_IMAGES, RESAMPLE_MAX_SIDE = CONSTANTS["ZIRA_RESAMPLE_MAX_IMAGES"], CONSTANTS["ZIRA_RESAMPLE_MAX_SIDE"]
RESAMPLE_MAX_TAPS = CONSTANTS["ZIRA_RESAMPLE_MAX_TAPS"]
# The second public header, the metrics log's (metrics.py), in tables of its own: the ones above are zira_msda.h's alone.
METRICS_PROTOTYPES, METRICS_STRUCTS, METRICS_CONSTANTS = read_header(_METRICS_HEADER)
METRICS_SYMBOLS = tuple(METRICS_PROTOTYPES)
MetricsSources = METRICS_STRUCTS["zira_metrics_sources"]
# The third, the multilayer-branch epilogue's (rsb_multilayer.py): prototypes only.
RSB_ML_PROTOTYPES = read_header(_RSB_ML_HEADER)[0]
RSB_ML_SYMBOLS = tuple(RSB_ML_PROTOTYPES)
# The fourth, the batched box NMS's (nms.py): prototypes and its two limits.
NMS_PROTOTYPES, _, NMS_CONSTANTS = read_header(_NMS_HEADER)
NMS_SYMBOLS = tuple(NMS_PROTOTYPES)
NMS_MAX_K, NMS_MAX_B = NMS_CONSTANTS["ZIRA_NMS_MAX_K"], NMS_CONSTANTS["ZIRA_NMS_MAX_B"]
# The fifth, the chunked vocabulary's merged detections tail (vocab.py): prototypes, limits and the chunk table.
VOCAB_PROTOTYPES, VOCAB_STRUCTS, VOCAB_CONSTANTS = read_header(_VOCAB_HEADER)
VOCAB_SYMBOLS = tuple(VOCAB_PROTOTYPES)
VocabChunks = VOCAB_STRUCTS["zira_vocab_chunks"]
# The sixth, the LVIS box AP matching's (lvis_evaluation.py): prototypes and its four limits.
LVIS_PROTOTYPES, _, LVIS_CONSTANTS = read_header(_LVIS_HEADER)
LVIS_SYMBOLS = tuple(LVIS_PROTOTYPES)
# The seventh, the phrase-grounding matching's (phrase_evaluation.py): prototypes and its seven limits.
PHRASE_PROTOTYPES, _, PHRASE_CONSTANTS = read_header(_PHRASE_HEADER)
PHRASE_SYMBOLS = tuple(PHRASE_PROTOTYPES)
# The eighth, the gated adapter's (adapter.py): prototypes only.
ADAPTER_PROTOTYPES = read_header(_ADAPTER_HEADER)[0]
ADAPTER_SYMBOLS = tuple(ADAPTER_PROTOTYPES)
# The ninth, the trained class head's of the linear-probing baseline (utils.py): prototypes only.
CLSLINEAR_PROTOTYPES = read_header(_CLSLINEAR_HEADER)[0]
CLSLINEAR_SYMBOLS = tuple(CLSLINEAR_PROTOTYPES)
# The tenth, the prompt-tuning baseline's substitution (prompt.py): prototypes, its five limits and the segment table's row.
PROMPT_PROTOTYPES, PROMPT_STRUCTS, PROMPT_CONSTANTS = read_header(_PROMPT_HEADER)
PROMPT_SYMBOLS = tuple(PROMPT_PROTOTYPES)
PromptSegment = PROMPT_STRUCTS["zira_prompt_segment"]
# The eleventh, the text-memory replay's loss (prompt.py, memory_loss): prototypes only; limits and tables are the tenth's.
PMEM_PROTOTYPES = read_header(_PMEM_HEADER)[0]
PMEM_SYMBOLS = tuple(PMEM_PROTOTYPES)
# The twelfth, the CET text adapter's (cet.py): prototypes and its limits and loss codes.
CET_PROTOTYPES, _, CET_CONSTANTS = read_header(_CET_HEADER)
CET_SYMBOLS = tuple(CET_PROTOTYPES)
# The thirteenth, the low-rank language side branch's (rsb.py, RepZeroLoRA): prototypes and its limits.
LORA_PROTOTYPES, _, LORA_CONSTANTS = read_header(_LORA_HEADER)
LORA_SYMBOLS = tuple(LORA_PROTOTYPES)

_lib = None


class ExtensionMissingError(ImportError):
    pass


def assert_int64_rows(struct, names):
    """An ``[n, len(names)]`` int64 tensor is a ``struct[]``: these fields in this order, 8 bytes each, no padding."""
    fields = [(name, ctypes.sizeof(ctype)) for name, ctype in struct._fields_]
    assert fields == [(name, 8) for name in names] and ctypes.sizeof(struct) == 8 * len(names), (struct.__name__, fields)


def load():
    """Load (once) and return the ctypes handle of libzira_msda.so, every entry point typed as the header declares it."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ExtensionMissingError(
            "HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or python -m ziragroundingdino_amd.build). There is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in (list(PROTOTYPES.items()) + list(METRICS_PROTOTYPES.items()) + list(RSB_ML_PROTOTYPES.items())
                                      + list(NMS_PROTOTYPES.items()) + list(VOCAB_PROTOTYPES.items())
                                      + list(LVIS_PROTOTYPES.items()) + list(PHRASE_PROTOTYPES.items())
                                      + list(ADAPTER_PROTOTYPES.items()) + list(CLSLINEAR_PROTOTYPES.items())
                                      + list(PROMPT_PROTOTYPES.items()) + list(PMEM_PROTOTYPES.items())
                                      + list(CET_PROTOTYPES.items()) + list(LORA_PROTOTYPES.items())):
        f = getattr(lib, name)
        f.argtypes, f.restype = argtypes, restype
    _lib = lib
    return lib


def version():
    return load().zira_msda_version().decode()


def variant_f32(D):
    return load().zira_msda_variant_f32(int(D)).decode()
