"""The opt-in products behind pipeline.predict_and_fuse, stated once: PRODUCTS lists them in the order the pipeline runs them.

A row is a dict:
    "name"    the keyword of predict_and_fuse and the flag of predict (--<name> PATH; its settings are --<name>_*)
    "needs"   ((product, reason), ...): what must be on too.  "fuse" is predict's --fuse: predict_and_fuse is that step itself
    "parts"   ((flag, attribute of the parsed arguments that is not None when the part is on, reason), ...): nested steps with
              flags of their own, which need this product; in a settings dict they are keys of the product's own dict
    "check"   the function that checks the product's settings dict (a ValueError in the stage's words)
    "report"  ((timing key, the path's attribute or None, text), ...): the lines predict prints on rank 0, in order, each for a key
              that predict_and_fuse's `timings` received; the first key is the product's own, the others are parts of it
predict_and_fuse raises "<name> needs <product>: <reason>" (check), predict.parse_args says "--<name> needs --<product> (<reason>)"
(check_args), and predict.main prints report_lines.  What does not fit a row stays explicit code beside the walk: a DSM from the
mesh needs the mesh, the cloud's colours tie it to the "views" partition, and the borders and units predict fills in."""
from . import cloud, dsm, dtm, mesh, objects, ortho, ortho_mesh, refine, texture


def _check_mesh(s):
    mesh.check_settings(mesh.MeshGrid(s["border"], s["voxel"]), s.get("trunc"), s.get("min_views", mesh.DEFAULT_MIN_VIEWS),
                        s.get("conf_threshold", mesh.DEFAULT_CONF), s.get("views_per_batch"))
    mesh.edit_settings(s)
    if s.get("refine") is not None:
        refine.check_refine_settings(s["refine"])


def _check_dsm(s):
    source = s.get("source", "pc")
    if source not in dsm.SOURCES:
        raise ValueError("dsm source %r: 'pc' or 'mesh'" % (source,))
    if source == "mesh":
        dsm.check_mesh_settings(s)


def _check_ortho(s):
    ortho.check_tolerance(s.get("depth_tolerance", ortho.DEFAULT_TOLERANCE))
    ortho.check_views_per_batch(s.get("views_per_batch"))


def _check_texture(s):
    texture.check_settings(s)
    for key, check in (("level", texture.check_level_settings), ("local", texture.check_local_settings), ("ortho", ortho_mesh.check_settings)):
        if s.get(key) is not None:
            check(s[key])


def _outliers_line(o):
    return "cloud outliers: kept %d of %d points, dropped %d" % (o["kept"], o["points"], o["points"] - o["kept"])


PRODUCTS = (
    {"name": "cloud", "needs": (("fuse", "the cloud is merged from the fused points"),),
     "parts": (("cloud_outlier_radius", "cloud_outlier_radius", "it is the merged cloud that is cleaned"),),
     "check": cloud.check_settings,   # checks the outlier filter's settings too
     "report": (("cloud_s", "cloud", "merged point cloud %s"), ("cloud_outliers", None, _outliers_line))},
    {"name": "mesh", "needs": (("fuse", "the mesh is built from the gathered depth maps of the fusion step"),),
     "parts": (("mesh_collapse", "mesh_collapse_min_edge", "it is the mesh whose edges are collapsed"),
               ("mesh_flip", "mesh_flip_max_angle", "it is the mesh whose edges are flipped"),
               ("mesh_refine", "mesh_refine_step", "it is the mesh that is refined")), "check": _check_mesh,
     "report": (("mesh_s", "mesh", "mesh %s"), ("mesh_collapse_s", None, "mesh edges the views cannot resolve collapsed"),
                ("mesh_flip_s", None, "mesh edges flipped to remove cap triangles"),
                ("mesh_subdivide_s", None, "mesh subdivided against the views"), ("mesh_refine_s", None, "mesh refined against the images"))},
    {"name": "dsm", "needs": (("fuse", "the DSM is built from the fused points"),), "parts": (), "check": _check_dsm,
     "report": (("dsm_s", "dsm", "DSM %s"),)},
    {"name": "ortho", "needs": (("fuse", "the orthophoto is draped on the DSM of the fused points"), ("dsm", "the orthophoto is draped on the DSM")),
     "parts": (), "check": _check_ortho, "report": (("ortho_s", "ortho", "orthophoto %s"),)},
    {"name": "dtm", "needs": (("dsm", "the terrain is filtered from the DSM"),), "parts": (), "check": dtm.check_settings,
     "report": (("dtm_s", "dtm", "DTM %s"),)},
    {"name": "objects", "needs": (("dtm", "the objects are segmented from the nDSM the terrain step returns"),), "parts": (),
     "check": objects.check_settings, "report": (("objects_s", "objects", "objects %s"),)},
    {"name": "texture", "needs": (("fuse", "the mesh is textured from the views of the fusion step"), ("mesh", "the texture is laid on the mesh")),
     "parts": (("texture_ortho", "texture_ortho", "the orthophoto is rendered from the textured mesh"),), "check": _check_texture,
     "report": (("texture_s", "texture", "textured mesh %s"), ("texture_ortho_s", "texture_ortho", "orthophoto of the textured mesh %s"))},
)
NAMES = tuple(p["name"] for p in PRODUCTS)
REPORT_ORDER = ("cloud", "dsm", "dtm", "objects", "ortho", "mesh", "texture")   # the order of predict's lines: not the order the products run in


def check(settings):
    """The up-front checks of predict_and_fuse: settings maps every product's name to its settings dict or None.  Every product
    that is on has what it needs, then its settings pass its check, in the pipeline's order."""
    for p in PRODUCTS:
        if settings[p["name"]] is not None:
            for need, reason in p["needs"]:
                if need != "fuse" and settings[need] is None:
                    raise ValueError("%s needs %s: %s" % (p["name"], need, reason))
            p["check"](settings[p["name"]])


def check_args(ap, a):
    """The same dependencies on predict's parsed arguments, reported through ap.error."""
    for p in PRODUCTS:
        if getattr(a, p["name"]) is not None:
            for need, reason in p["needs"]:
                if not a.fuse if need == "fuse" else getattr(a, need) is None:
                    ap.error("--%s needs --%s (%s)" % (p["name"], need, reason))
        for flag, attr, reason in p["parts"]:
            if getattr(a, attr) is not None and getattr(a, p["name"]) is None:
                ap.error("--%s needs --%s (%s)" % (flag, p["name"], reason))


def report_lines(a, timings, world):
    """The lines predict.main prints on rank 0 for the products that are on, from the timings predict_and_fuse filled."""
    by_name = {p["name"]: p for p in PRODUCTS}
    for name in REPORT_ORDER:
        for key, attr, text in by_name[name]["report"] if getattr(a, name) is not None else ():
            if key in timings:
                line = text(timings[key]) if callable(text) else (text % getattr(a, attr) if attr else text) + " in %.2f s" % timings[key]
                yield "rank 0/%d: %s" % (world, line)
