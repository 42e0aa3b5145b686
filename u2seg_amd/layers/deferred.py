"""Registry of the gradients that a backward node hands on as a placeholder instead of a tensor.

Three backward-pass folds in layers/functional.py let ANOTHER autograd node finish a gradient: the node that would have produced it
posts what the consumer needs (`post`) and returns a one-element zero tensor expanded to the gradient's shape; the consumer
recognises that placeholder by its device address (`take`) and launches the kernel that forms the real thing.  A placeholder that
meets anything else - a second consumer, a sum autograd formed, a pass that raised midway - would be a silently wrong gradient, so
every entry is accounted for: `pending` / `drain` are what the guards and the start and end of a training step check.

Nothing here launches a kernel or needs a GPU; the payloads are opaque.
"""
import torch

BN_APPLY = "bn_apply"      # payload (dz, y, coef): the batch-norm backward apply step, left to the producing 1x1 conv's backward
ROI_GATHER = "roi_gather"  # payload (shared, level): the ROIAlign gather of an FPN map, left to the map's fan-out node
TAIL = "tail"              # payload the tail's state: (dz, sums) of a residual tail, formed by the next block's conv1 data gradient
KINDS = (BN_APPLY, ROI_GATHER, TAIL)
SLOTS = 64

_entries = {}                     # (device index, placeholder address) -> (kind, placeholder, payload); keeps both alive
_count = dict.fromkeys(KINDS, 0)  # entries per kind: what lets take() / holds() answer without asking for an address
# device index -> [zero-filled bf16 pool, next slot].  Placeholders are ZEROS, so that a sum autograd forms with one by accident is
# numerically the other addend (and no longer has the placeholder's address: the guards and the checks of a step's ends catch it)
_pools = {}


def _key(t):
    return (t.device.index, t.data_ptr())


def post(kind, device, shape, payload):
    """Record `payload` under a free slot of the device's pool; returns that slot expanded to `shape`."""
    pool = _pools.get(device.index)
    if pool is None:
        pool = _pools[device.index] = [torch.zeros(SLOTS, dtype=torch.bfloat16, device=device), 0]
    for _ in range(SLOTS):
        slot = pool[0][pool[1] : pool[1] + 1]
        pool[1] = (pool[1] + 1) % SLOTS
        if _key(slot) not in _entries:
            ph = slot.expand(shape)
            _entries[_key(slot)] = (kind, ph, payload)
            _count[kind] += 1
            return ph
    raise RuntimeError("%d deferred gradients were not consumed by their consumers" % sum(drain().values()))


def holds(kind, grad, posted=None):
    """Is `grad` a pending placeholder of that kind (and, with `posted`, the very tensor that post() returned)?  By address: a
    placeholder that autograd summed with something lives elsewhere."""
    if not _count[kind]:
        return False
    ent = _entries.get(_key(grad))
    return ent is not None and ent[0] == kind and (posted is None or ent[1] is posted)


def take(kind, grad):
    """The payload posted under `grad` if it is a pending placeholder of that kind (the entry is removed), else None.  Runs in
    every convolution's and fan-out node's backward: with nothing of the kind pending it costs one dict lookup."""
    if not _count[kind] or not holds(kind, grad):
        return None
    _count[kind] -= 1
    return _entries.pop(_key(grad))[2]


def pending():
    """{kind: entries posted and not yet taken}"""
    return dict(_count)


def drain():
    """Forget every entry; returns what pending() said."""
    dropped = pending()
    _entries.clear()
    _count.update(dict.fromkeys(KINDS, 0))
    return dropped
