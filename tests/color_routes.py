"""The reference's colour routing, written down a third time and on purpose by hand: `<Space>(T).to(target)` of src/color.zig as a table, and
convertColor's rule for when the component type changes. colorspaces.hip (`next_hop`) and oracle/colorspaces_impl.h (`cs_to`) are the other
two restatements; this one was transcribed from the reference's switch statements, not from either, so that the tests which walk it
(tests/test_color_routes.py, tests/test_gpu_color_pairs.py) can tell a wrong hub in one of them from a shared misreading.

A space is named as the reference's ColorSpace tag in capitals, a form is (space, "u8" | "f32"): the Zig pixel type."""
import numpy as np

# a row is ({target: the space the value is in after ONE conversion function}, the `else =>` hub); `.x => self` is left out
_ROWS = {
    "RGB": ({"GRAY": "GRAY", "HSL": "HSL", "HSV": "HSV", "RGBA": "RGBA", "XYB": "XYB", "XYZ": "XYZ", "YCBCR": "YCBCR"}, "XYZ"),  # color.zig:350-361
    "RGBA": ({"RGB": "RGB"}, "RGB"),                                                                                           # :475-480
    "GRAY": ({}, "RGB"),                                                                          # :533-537, grayToRgb(self).to(target)
    "HSV": ({"HSL": "HSL", "RGB": "RGB"}, "RGB"),                                                                              # :586-592
    "HSL": ({"HSV": "HSV", "RGB": "RGB"}, "RGB"),                                                                              # :624-630
    "XYZ": ({"LAB": "LAB", "LCH": "LAB", "LMS": "LMS", "OKLAB": "OKLAB", "OKLCH": "OKLAB", "RGB": "RGB", "XYB": "XYB"}, "RGB"),  # :667-678
    "LAB": ({"LCH": "LCH", "XYZ": "XYZ"}, "XYZ"),                                                                              # :711-717
    "LCH": ({"LAB": "LAB"}, "LAB"),                                                                                            # :750-755
    "LMS": ({"XYZ": "XYZ"}, "XYZ"),                                                                                            # :786-791
    "OKLAB": ({"OKLCH": "OKLCH", "XYZ": "XYZ"}, "XYZ"),                                                                        # :824-830
    "OKLCH": ({"OKLAB": "OKLAB"}, "OKLAB"),                                                                                    # :863-868
    "XYB": ({"RGB": "RGB", "XYZ": "XYZ"}, "XYZ"),                                                                              # :902-908
    "YCBCR": ({"RGB": "RGB"}, "RGB"),                                                                                          # :943-948
}
SPACES = tuple(sorted(_ROWS))
NEXT_HOP = {cur: {to: named.get(to, hub) for to in SPACES if to != cur} for cur, (named, hub) in _ROWS.items()}

U8_SPACES = ("GRAY", "RGB", "RGBA", "YCBCR")  # the types that accept a u8 backing (color.zig:280-284, 394-398, 516-520, 925-929)
FORMS = tuple((s, t) for s in U8_SPACES for t in ("u8", "f32")) + tuple((s, "f32") for s in SPACES if s not in U8_SPACES)
HUE_FIELD = {"HSL": 0, "HSV": 0, "LCH": 2, "OKLCH": 2}


def channels(space):
    return 1 if space == "GRAY" else (4 if space == "RGBA" else 3)


def route(cur, to):
    """The spaces a value passes through after `cur`, `to` last; [] when there is nothing to do."""
    out = []
    while cur != to:
        cur = NEXT_HOP[cur][to]
        out.append(cur)
        assert len(out) <= 8, (out, to)
    return out


def form_route(src, dst):
    """convertColor(Dest, source) (color.zig:108-151) as the forms after each single step, `dst` last. A scalar image is a grey whose
    component type changes FIRST (:128-130); a colour going to a scalar is routed in its own type and cast last (:135); a colour going to a
    float colour is cast first (:145-148); everything else is routed in its own type and cast last (:150)."""
    (ss, st), (ds, dt) = src, dst
    if ss == ds:
        return [] if st == dt else [dst]
    if ss == "GRAY" or (dt == "f32" and ds != "GRAY"):
        return ([(ss, dt)] if st != dt else []) + [(s, dt) for s in route(ss, ds)]
    return [(s, st) for s in route(ss, ds)] + ([dst] if st != dt else [])


def lattice_frame(rows, cols):
    """rows x cols Rgb(u8) colours: the 16-step lattice (4096 colours: sixteen greys, black, white and the cube's other corners among
    them), then colours of the 64-step lattice at a stride that is coprime to 64, so every channel keeps moving."""
    n = rows * cols
    assert n > 4096
    coarse, fine = (np.linspace(0, 255, k).round().astype(np.uint8) for k in (16, 64))
    cube16 = np.stack(np.meshgrid(coarse, coarse, coarse, indexing="ij"), -1).reshape(-1, 3)
    cube64 = np.stack(np.meshgrid(fine, fine, fine, indexing="ij"), -1).reshape(-1, 3)
    step = (64 ** 3 // (n - 4096)) | 1
    return np.ascontiguousarray(np.concatenate([cube16, cube64[::step][: n - 4096]]).reshape(rows, cols, 3))
