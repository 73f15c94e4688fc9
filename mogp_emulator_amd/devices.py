"""
Which GPUs a ``MultiOutputGP_GPU`` spreads its emulators over (``devices=`` of the class and of ``fit_GP_MAP``).

Pure Python with no import of the native library, so that it can be checked without a GPU.  The split itself is the one
of ``dist.shard_bounds``: contiguous blocks of ceil(n_emulators / n_devices) emulators, one part per non-empty block.
"""
import numbers
import os

ENV = "MOGP_DEVICES"


def parse_devices(devices, n_visible, environ=None):
    """The device list of a model, or None for today's single engine on the current device.

    devices: None, "all", a string "0,1,..." or a sequence of ordinals.  None reads the environment variable MOGP_DEVICES
    (same forms) from `environ` (default os.environ); when that is unset or empty the result is None.  n_visible: number of
    visible GPUs.  Bad input raises ValueError."""
    if devices is None:
        spec = (os.environ if environ is None else environ).get(ENV, "")
        if not spec.strip():
            return None
        devices = spec
    if isinstance(devices, str):
        spec = devices.strip()
        if spec.lower() == "all":
            if int(n_visible) < 1:
                raise ValueError("devices='all': no GPU is visible")
            return list(range(int(n_visible)))
        items = [p.strip() for p in spec.split(",")]
        if not spec or any(not p for p in items):
            raise ValueError("devices must be 'all' or a comma-separated list of device ordinals, not %r" % devices)
        try:
            out = [int(p) for p in items]
        except ValueError:
            raise ValueError("devices must be 'all' or a comma-separated list of device ordinals, not %r" % devices)
    else:
        try:
            items = list(devices)
        except TypeError:
            raise ValueError("devices must be None, 'all' or a sequence of device ordinals, not %r" % (devices,))
        out = []
        for d in items:
            if isinstance(d, bool) or not isinstance(d, numbers.Integral):
                raise ValueError("device ordinals must be integers, not %r" % (d,))
            out.append(int(d))
    if not out:
        raise ValueError("devices must name at least one device")
    for d in out:
        if d < 0 or d >= int(n_visible):
            raise ValueError("device ordinal %d is out of range [0, %d)" % (d, int(n_visible)))
    return out


def split_bounds(n_items, n_devices):
    """[(part index, lo, hi)] of the non-empty contiguous blocks -- the parts a model on `n_devices` devices is made of."""
    per = -(-int(n_items) // int(n_devices))
    out = []
    for k in range(int(n_devices)):
        lo = min(k * per, int(n_items))
        hi = min(lo + per, int(n_items))
        if lo < hi:
            out.append((k, lo, hi))
    return out
