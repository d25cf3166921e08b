"""tools/variants.py against the sources it builds variants of: every macro a
variant sets is one the sources read, and every timing patch still finds its
anchor, exactly once, in the file it patches."""
import importlib.util
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "heatmap_amd", "csrc")


def _variants():
    spec = importlib.util.spec_from_file_location("hm_tools_variants", os.path.join(REPO, "tools", "variants.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC))}


def test_variant_macros_occur_in_sources():
    v = _variants()
    text = "\n".join(_sources().values())
    words = set(re.findall(r"\bHM_[A-Z0-9_]+\b", text))
    defines = {(name, d) for name, ds in list(v.VARIANTS.items()) + list(v.PATCH_DEFINES.items()) for d in ds}
    assert defines
    missing = sorted((name, d) for name, d in defines if d.split("=", 1)[0] not in words)
    assert not missing, "variants that set a macro no source mentions: %r" % missing


def test_patch_anchors_occur_exactly_once():
    v = _variants()
    src = _sources()
    assert v.PATCHES
    bad = []
    for name, patches in v.PATCHES.items():
        for f, old, new in patches:
            n = src[f].count(old) if f in src else -1
            if n != 1:
                bad.append((name, f, n, old.splitlines()[0].strip()))
            assert old != new, name
    assert not bad, "patch anchors that do not occur exactly once (name, file, occurrences, first line): %r" % bad
