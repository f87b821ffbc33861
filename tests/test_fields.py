"""CPU: field channels in the scene description, the scene reader / writer and the EXR writer (the reference's `multichannel` integrator with nested `field`
integrators, src/integrators/misc/multichannel.cpp, field.cpp; the film's pixelFormat / channelNames lists, src/films/hdrfilm.cpp:215-263)."""
import importlib
import os
import numpy as np
import pytest
from tests.conftest import GOLDEN

X = importlib.import_module("mitsuba-im_amd.xml_scene")
S = importlib.import_module("mitsuba-im_amd.scenes")
A = importlib.import_module("mitsuba-im_amd.api")
R = importlib.import_module("mitsuba-im_amd.render")
imageio = importlib.import_module("mitsuba-im_amd.imageio")
XML = os.path.join(GOLDEN, "scenes", "multichannel_fields.xml")

BODY = """<sensor type="perspective"><film type="hdrfilm"><integer name="width" value="16"/><integer name="height" value="8"/>{film}</film></sensor>
<shape type="rectangle"><emitter type="area"><spectrum name="radiance" value="3"/></emitter></shape></scene>"""
FIELD = '<integrator type="field"><string name="field" value="{0}"/></integrator>'


def load_text(tmp_path, integrator, film=""):
    p = tmp_path / "s.xml"; p.write_text('<scene version="0.5.0">' + integrator + BODY.format(film=film))
    return X.load_scene(str(p))


def test_multichannel_scene_file():
    sc = X.load_scene(XML)
    assert sc.integrator == S.INTEGRATOR_PATH and sc.max_depth == 4 and (sc.width, sc.height, sc.filter) == (32, 24, S.FILTER_BOX)
    assert sc.fields == [("shNormal", (0.0, 0.0, 0.0)), ("distance", (-1.0, -1.0, -1.0))]
    assert sc.pixel_formats == ["rgb", "rgb", "luminance"] and sc.channel_names == ["color", "normal", "distance"]
    assert S.cornell_box(width=8, height=8).fields == []                                   # empty by default


def test_undefined_value_kinds(tmp_path):
    integ = ('<integrator type="multichannel"><integrator type="volpath"/>'
             '<integrator type="field"><string name="field" value="uv"/><rgb name="undefined" value="0.25, 0.5, 2"/></integrator>'
             '<integrator type="field"><string name="field" value="primIndex"/><spectrum name="undefined" value="3"/></integrator></integrator>')
    sc = load_text(tmp_path, integ)
    assert sc.integrator == S.INTEGRATOR_VOLPATH and sc.fields == [("uv", (0.25, 0.5, 2.0)), ("primIndex", (3.0, 3.0, 3.0))]
    assert sc.pixel_formats == ["rgb"] * 3 and sc.channel_names == []                       # nothing said in the film: defaults
    assert A.normalize_fields(["albedo", ("distance", 2), ("uv", (1, 2, 3))]) == [("albedo", (0.0,) * 3), ("distance", (2.0,) * 3), ("uv", (1.0, 2.0, 3.0))]
    with pytest.raises(ValueError, match="unknown field"):
        A.normalize_fields(["depth"])


@pytest.mark.parametrize("integrator,film,message", [
    (FIELD.format("distance"), "", "at the root is not supported"),
    ('<integrator type="multichannel"><integrator type="path"/><integrator type="volpath"/>' + FIELD.format("uv") + "</integrator>", "", "exactly one radiance integrator"),
    ('<integrator type="multichannel">' + FIELD.format("uv") + "</integrator>", "", "exactly one radiance integrator"),
    ('<integrator type="multichannel"><integrator type="path"/>' + FIELD.format("depth") + "</integrator>", "",
     "must be one of position, relPosition, distance, geoNormal, shNormal, uv, albedo, shapeIndex, primIndex"),
    ('<integrator type="multichannel"><integrator type="path"/>' + FIELD.format("uv") + "</integrator>",
     '<string name="pixelFormat" value="rgb, rgb, rgb"/><string name="channelNames" value="a, b, c"/>', "one entry per nested integrator"),
    ('<integrator type="multichannel"><integrator type="path"/>' + FIELD.format("uv") + "</integrator>",
     '<string name="pixelFormat" value="rgb, rgb"/><string name="channelNames" value="a"/>', "Number of channel names must match"),
    ('<integrator type="multichannel"><integrator type="path"/>' + FIELD.format("uv") + "</integrator>",
     '<string name="pixelFormat" value="rgb, xyz"/><string name="channelNames" value="a, b"/>', 'pixelFormat "xyz" is not supported'),
    ('<integrator type="multichannel"><integrator type="bdpt"/>' + FIELD.format("uv") + "</integrator>", "", 'integrator "bdpt" is not supported'),
])
def test_scene_file_errors(tmp_path, integrator, film, message):
    with pytest.raises(X.SceneError) as e:
        load_text(tmp_path, integrator, film)
    assert message in str(e.value)


def test_export_round_trips_the_fields(tmp_path):
    sc = S.cornell_box(width=16, height=8, spp=2); sc.fields = ["shNormal", ("distance", -1.0), ("uv", (0.5, 0.25, 2.0))]
    path = X.export_scene(sc, str(tmp_path), "fields")
    back = X.load_scene(path if isinstance(path, str) else str(tmp_path / "fields.xml"))
    assert back.fields == A.normalize_fields(sc.fields) and back.integrator == S.INTEGRATOR_PATH and back.max_depth == sc.max_depth
    assert back.pixel_formats == ["rgb"] * 4 and back.channel_names == ["color", "shNormal", "distance", "uv"]
    src = X.load_scene(XML); X.export_scene(src, str(tmp_path), "again"); again = X.load_scene(str(tmp_path / "again.xml"))     # the film's own lists survive
    assert again.fields == src.fields and again.pixel_formats == src.pixel_formats and again.channel_names == src.channel_names
    plain = X.load_scene(X.export_scene(S.cornell_box(width=16, height=8, spp=2), str(tmp_path), "plain") or str(tmp_path / "plain.xml"))
    assert plain.fields == []


def test_exr_with_field_channel_groups(tmp_path):
    rng = np.random.default_rng(5); rgb = rng.random((6, 9, 3)).astype(np.float32); fl = rng.normal(size=(6, 9, 6)).astype(np.float32)
    fl[..., 3:] = fl[..., 3:4]                                                             # a scalar field: three equal values
    sc = S.Scene(channel_names=["color", "normal", "distance"], pixel_formats=["rgb", "rgb", "luminance"])
    planes, chan = R.field_channel_groups(sc, rgb, fl, ["shNormal", "distance"])
    assert chan == ["color.R", "color.G", "color.B", "normal.R", "normal.G", "normal.B", "distance.Y"]
    out = str(tmp_path / "f.exr"); imageio.write_exr(out, planes, chan); pix, names = imageio.read_exr(out)
    assert sorted(names) == sorted(chan)
    got = {n: pix[..., i] for i, n in enumerate(names)}
    for i, c in enumerate("RGB"):
        assert (got["color." + c] == rgb[..., i]).all() and (got["normal." + c] == fl[..., i]).all()
    assert (got["distance.Y"] == fl[..., 3]).all()
    planes, chan = R.field_channel_groups(S.Scene(), rgb, fl, ["shNormal", "distance"])    # defaults: color, then the field kinds, all rgb
    assert chan == [g + "." + c for g in ("color", "shNormal", "distance") for c in "RGB"] and planes.shape == (6, 9, 9)
    with pytest.raises(ValueError):
        R.field_channel_groups(S.Scene(channel_names=["a"], pixel_formats=["rgb"]), rgb, fl, ["shNormal", "distance"])
