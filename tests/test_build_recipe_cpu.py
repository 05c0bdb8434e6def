"""No-GPU checks of the build recipe (hipbuild.py; no hipcc call): the shipped source set is the csrc/*.hip glob, every
instrumented preset links each source exactly once without touching a shipped object, and header edits trigger rebuilds."""
import os
from pathlib import Path

import pytest

from conftest import ROOT
import hipbuild

CSRC = Path(ROOT, "dawn-pytorch_amd", "csrc")
DROPPED = {}   # preset -> csrc stems it leaves out on purpose (none today)


def test_shipped_source_set_is_the_csrc_glob():
    assert hipbuild.sources() == sorted(CSRC.glob("*.hip"))
    assert {"dawn_api", "conv_gemm", "conv3x3_split", "gemm1x1_tiled", "gemm1x1_rows", "temporal_layer16"} <= {s.stem for s in hipbuild.sources()}
    assert [o for _, o, f in hipbuild.shipped_units()] == [Path(ROOT, "build", s.stem + ".o") for s in hipbuild.sources()]


@pytest.mark.parametrize("preset", sorted(hipbuild.PRESETS))
def test_preset_links_every_source_once(preset):
    units = hipbuild.preset_units(preset, ["-DDAWN_TL_TIMING"])
    shipped = {o for _, o, _ in hipbuild.shipped_units()}
    stems = [s.stem for s, _, _ in units if s.parent == CSRC]
    assert sorted(stems) == sorted({s.stem for s in hipbuild.sources()} - DROPPED.get(preset, set()))
    objs = [o for _, o, _ in units]
    assert len(set(objs)) == len(objs)
    for src, obj, flags in units:
        assert src.exists(), src
        if flags is None:
            assert obj in shipped
        else:
            assert obj not in shipped and obj.parent == Path(ROOT, "build", f"variant-{preset}"), obj
    assert any(f for _, _, f in units), "a preset recompiles at least one source with flags"


def test_presets_keep_their_flags_and_outputs():
    flags = {name: {s.stem: f for s, _, f in hipbuild.preset_units(name, ["-DX"]) if f is not None} for name in hipbuild.PRESETS}
    assert flags["sktiming"] == {"conv_gemm": ["-DDAWN_WITH_STREAMK"], "conv3x3_sk": ["-DDAWN_ABLATION"]}
    assert flags["tl16debug"] == {"temporal_layer16": ["-DX"]}
    assert flags["ablation"] == {"temporal_layer": ["-DDAWN_TL_TIMING"], "conv_gemm": ["-DDAWN_ABLATION"], "conv3x3_split": ["-DDAWN_ABLATION"],
                                 "gemm1x1_tiled": ["-DDAWN_ABLATION"], "gemm1x1_rows": ["-DDAWN_ABLATION"]}
    for p in hipbuild.PRESETS.values():
        assert p["out"].startswith("tools/ubench/") and p["out"].endswith(".bin")


def test_one_off_variant_and_unknown_source():
    units = hipbuild.variant_units("sla_layer", {"sla_layer": ["-DDAWN_SLA_OUT_FP32"]})
    assert [o for s, o, f in units if f] == [Path(ROOT, "build", "variant-sla_layer", "sla_layer.o")]
    with pytest.raises(RuntimeError):
        hipbuild.variant_units("x", {"no_such_source": []})


def test_header_change_triggers_rebuild(tmp_path):
    csrc, inc = tmp_path / "dawn-pytorch_amd" / "csrc", tmp_path / "include"
    (csrc / "sub").mkdir(parents=True)
    inc.mkdir()
    src, obj = csrc / "k.hip", tmp_path / "k.o"
    assert hipbuild.stale(obj, src, [])          # no object yet
    files = [src, csrc / "common.h", csrc / "sub" / "nested.h", inc / "api.h", obj]
    for i, p in enumerate(files):
        p.write_text("")
        os.utime(p, (1000 + i, 1000 + i))      # the object is the newest
    hdrs = hipbuild.headers(tmp_path)
    assert hdrs == sorted(files[1:4])
    assert not hipbuild.stale(obj, src, hdrs)
    for p in files[:4]:
        os.utime(p, (2000, 2000))
        assert hipbuild.stale(obj, src, hdrs), p
        os.utime(p, (1000, 1000))
