"""BASELINE config 5 end to end: sharded depth inference -> all-gather of the (depth, confidence) maps -> fusion.

The reference runs the two steps as separate programs that meet on disk: predict.py writes {name}_init.pfm / _prob.pfm /
.txt per reference view (predict.py:146-183), fuse/fusion_3d_normal.py:404-533 reads them back view by view.  Here the
maps never leave HBM:

    rank r:  predict_views(keep_maps=True) over ITS views      (sharding.shard_views; the PFM products are still written)
             all_gather_maps([n_local, 2, H, W])               (the ONE collective of the path: RCCL over xGMI, gloo when
                                                                ranks share a card) + the views' [2,4,4] cameras
             fuse.fuse_block over ITS reference views           (sources looked up in the gathered maps)
             fuse.extract_points per reference view

Ownership rule: the rank that sweeps a reference view also fuses it (the same contiguous blocks of `viewpair.txt` order,
sharding.shard_views), against the gathered maps of ALL views.  What this preserves of the reference:

* With `filter_sources=False` every reference view is fused against the unmodified depth maps: results do not depend on the
  order of the views, so the union over ranks is bit for bit the single-rank result (tests/test_pipeline_gpu.py).
* With `filter_sources=True` (the reference's default, save_temp: fusion_3d_normal.py:417-418, 479-480, 504-510, 529-533)
  a source map loses the samples a reference view has confirmed before the NEXT reference view reads it -- a chain through
  the whole view list of a scene block.  A rank runs that chain over its own reference views in list order, starting from
  the unfiltered gathered maps: inside a rank's block of views the reference's behaviour is kept exactly; samples confirmed
  by reference views of LOWER ranks are still offered (duplicate points along the seams between rank blocks).  One rank
  reproduces the reference's chain over the whole list.

* `fuse_partition="scene_blocks"` (with the scene blocks of blocks.txt, dataset.read_scene_blocks): the reference fuses scene
  block by scene block and starts the chain afresh for each (fusion_3d_normal.py:593-608; the tmp folder is emptied at the end
  of fuse_depths, :586-587).  Scene blocks are therefore the units whose chains are INDEPENDENT: dealt whole to the ranks
  (block b to rank b mod N -- fusion ownership then differs from sweep ownership, which costs nothing: every rank holds every
  map after the gather) they reproduce the reference's result exactly for any N, filtering on, vertices clipped to each block's
  scene range as :557 does.  Balanced only when there are at least N blocks; the default partition ("views") always is.

The view list, the sources of a view (all the sources viewpair.txt lists, up to `fusion_num` -- the fusion step does not stop
at predict's view_num: fusion_3d_normal.py:98, 476) and the 1-based image ids of the visibility lists come from the dataset
(`view_records`); cameras are the `outcam` of the item whose reference view the image is -- what the reference reads back from
{name}.txt (fusion_3d_normal.py:425-427; write_red_cam's str(float32) round-trips exactly).
"""
import os
import time

import numpy as np
import torch
import torch.distributed as dist

from . import (cloud as _cloud, dsm as _dsm, dtm as _dtm, fuse, mesh as _mesh, objects as _objects, ortho as _ortho, ortho_mesh as _om,
               predict, products, refine as _refine, sharding, texture as _tx)
from ._geom import timed


def view_records(dataset, fusion_num=10):
    """[{"name", "src": [names], "id"}] for every item of the dataset, by item index -- metadata only (no image is read).
    Datasets provide `view_records(fusion_num)`: dataset.MVSDataset / DeviceItems from viewpair.txt + images.txt,
    predict.SyntheticStrip from its ring."""
    fn = getattr(dataset, "view_records", None)
    if fn is None:
        raise TypeError("%s has no view_records(): the fusion step needs the view list of the block" % type(dataset).__name__)
    recs = fn(fusion_num)
    if len(recs) != len(dataset):
        raise ValueError("view_records() lists %d views, the dataset has %d items" % (len(recs), len(dataset)))
    return recs


def _gather_objects(obj, world_size):
    if world_size == 1:
        return [obj]
    out = [None] * world_size
    dist.all_gather_object(out, obj)
    return out


def predict_and_fuse(model, dataset, output_folder, rank=0, world_size=1, checker=None, fusion_num=10, min_geo_consist_num=4,
                     filter_sources=True, partition="block", scene_range=None, skip_line=2, feature_cache_bytes=0,
                     device="cuda", timings=None, display=False, fuse_partition="views", scene_blocks=None,
                     estimate_normals=False, normal_nei=1, save_normals=False, dsm=None, ortho=None, mesh=None, texture=None,
                     dtm=None, objects=None, cloud=None):
    """Runs the three steps above for this rank.  Returns a list, one entry per reference view this rank owns, of
    {"ref", "final_mask" [H,W] bool, "avg_xyz_world" [3,H,W], "points": fuse.extract_points(...) dict} (device tensors).
    timings: dict that receives predict_s, allgather_ms (the collective alone, synchronised on both sides), fuse_s.
    estimate_normals, normal_nei: the views' normal maps are estimated from their depth maps (add_estimated_normals) instead of the
    default (0, 0, -1).  save_normals: predict_views also writes {name}_normal.pfm.
    The products (products.PRODUCTS, in the order they run) are each None (nothing changes: no file, no collective, no timing key) or
    a settings dict; what one needs of another and every settings dict are checked before the model or the dataset is touched:
    cloud:   the merged coloured point cloud (write_cloud_of); timings gets cloud_s.
    mesh:    the surface mesh with its edit steps and refinement, on rank 0 (write_mesh_of, gather_refine_views); mesh_s there.
    dsm:     the DSM of every rank's points (write_dsm_of) or, with "source": "mesh", of the mesh (write_mesh_dsm_of); dsm_s.
    ortho:   the true orthophoto on that DSM (write_ortho_of); ortho_s.
    dtm:     the terrain filtered from the DSM's raster, on rank 0 (write_dtm_of); dtm_s there.
    objects: the objects of the terrain step's nDSM, on rank 0 (write_objects_of); objects_s there.
    texture: the mesh textured from every rank's views, and its orthophoto (write_texture_of); texture_s."""
    if dsm is not None and dsm.get("source", "pc") == "mesh" and mesh is None:
        raise ValueError("a DSM from the mesh needs mesh settings: the DSM is rasterised from the mesh")
    products.check({"cloud": cloud, "mesh": mesh, "dsm": dsm, "ortho": ortho, "dtm": dtm, "objects": objects, "texture": texture})
    if cloud is not None and fuse_partition == "scene_blocks" and world_size > 1:
        raise ValueError("cloud with fuse_partition='scene_blocks' on %d ranks: the colours come from the reference crops of the "
                         "rank that swept the view (use fuse_partition='views')" % world_size)
    if checker is None:
        checker = fuse.ConsistencyChecker(1.0, 0.01, 90.0, 0.2)   # Fuse_Depth_Map's defaults (fusion_3d_normal.py:56-57)
    n = len(dataset)
    recs = view_records(dataset, fusion_num)
    mine = sharding.shard_views(n, rank, world_size, partition)
    cams = {}
    refine = mesh.get("refine") if mesh is not None else None
    images = {} if ortho is not None or texture is not None or refine is not None or cloud is not None else None
    t0 = time.perf_counter()
    maps = predict.predict_views(model, dataset, output_folder, rank, world_size, device=device, keep_maps=True,
                                 feature_cache_bytes=feature_cache_bytes, display=display, partition=partition, cams=cams,
                                 save_normals=save_normals, normal_nei=normal_nei, images=images)
    names = [recs[i]["name"] for i in mine]
    if list(maps.keys()) != names:
        raise RuntimeError("the views predict_views produced %s are not this rank's %s" % (list(maps.keys()), names))
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    # ---- every rank learns the map size (a rank may own no view) and the views agree on it
    shapes = _gather_objects([tuple(maps[k][0].shape) for k in names], world_size)
    sizes = {s for per in shapes for s in per}
    if len(sizes) != 1:
        raise ValueError("the maps of a block must share one size to be gathered (got %s)" % sorted(sizes))
    H, W = sizes.pop()
    dev = torch.device(device)
    if names:
        local = torch.stack([torch.stack([maps[k][0], maps[k][1]]) for k in names])
        local_cams = torch.from_numpy(np.stack([np.asarray(cams[k], np.float32) for k in names])).to(dev)
    else:
        local = torch.empty((0, 2, H, W), dtype=torch.float32, device=dev)
        local_cams = torch.empty((0, 2, 4, 4), dtype=torch.float32, device=dev)
    if world_size > 1:
        dist.barrier()
    torch.cuda.synchronize()
    g0 = time.perf_counter()
    all_maps = sharding.all_gather_maps(local, n, rank, world_size, partition)       # [n, 2, H, W], by global view index
    torch.cuda.synchronize()
    g1 = time.perf_counter()
    all_cams = sharding.all_gather_maps(local_cams, n, rank, world_size, partition).cpu().numpy()   # [n, 2, 4, 4]
    del local
    # ---- fusion of this rank's reference views against the gathered maps
    views = {}
    for i, r in enumerate(recs):
        views[r["name"]] = {"depth": all_maps[i, 0], "confidence": all_maps[i, 1], "K": all_cams[i, 1, :3, :3].copy(),
                            "E": all_cams[i, 0].copy(), "id": int(r["id"])}
    if fuse_partition not in ("views", "scene_blocks"):
        raise ValueError("fuse_partition must be 'views' or 'scene_blocks'")
    pair_of = lambda i: {"ref": recs[i]["name"], "src": list(recs[i]["src"])[:fusion_num]}

    def with_normals(pairs):
        if estimate_normals:
            add_estimated_normals(views, pairs, fusion_num, normal_nei)
        return pairs

    def ref_img(name):
        return reference_colors(images[name][1], H, W) if cloud is not None else None

    out = []
    if fuse_partition == "scene_blocks":
        if not scene_blocks:
            raise ValueError("fuse_partition='scene_blocks' needs the scene blocks (dataset.read_scene_blocks(blocks.txt))")
        by_image = {int(r.get("image", i)): i for i, r in enumerate(recs)}
        for b, blk in enumerate(scene_blocks):
            if b % world_size != rank:
                continue
            # (a reference view listed in a block but absent from the view list -- it had no sources -- has no maps: skipped with the
            #  warning the reference gives for a missing PFM, fusion_3d_normal.py:420-422)
            pairs = [pair_of(by_image[i]) for i in blk["refs"] if i in by_image]
            fused = fuse.fuse_block(views, with_normals(pairs), checker, fusion_num=fusion_num, min_geo_consist_num=min_geo_consist_num,
                                    filter_sources=filter_sources)
            for f in fused:
                pts = fuse.extract_points(f["avg_xyz_world"], f["final_mask"], f["vis_infos"], ref_img(f["ref"]), f["normal_world"],
                                          blk["scene_range"], skip_line)
                out.append({"ref": f["ref"], "scene": b, "final_mask": f["final_mask"], "avg_xyz_world": f["avg_xyz_world"], "points": pts})
    else:
        fused = fuse.fuse_block(views, with_normals([pair_of(i) for i in mine]), checker, fusion_num=fusion_num,
                                min_geo_consist_num=min_geo_consist_num, filter_sources=filter_sources)
        sr = scene_range if scene_range is not None else [-np.inf, np.inf, -np.inf, np.inf]
        for f in fused:
            pts = fuse.extract_points(f["avg_xyz_world"], f["final_mask"], f["vis_infos"], ref_img(f["ref"]), f["normal_world"], sr,
                                      skip_line)
            out.append({"ref": f["ref"], "final_mask": f["final_mask"], "avg_xyz_world": f["avg_xyz_world"], "points": pts})
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    if timings is not None:
        timings.update(views=len(mine), predict_s=t1 - t0, allgather_ms=(g1 - g0) * 1e3,
                       allgather_bytes=int(all_maps.numel() * 4), fuse_s=t2 - g1, map_size=(H, W),
                       backend=dist.get_backend() if world_size > 1 else "none")
    # this rank's [(id, K, E, depth, image)] in shard order: what the orthophoto and the texture take, and the refinement's images
    own = [(images[recs[i]["name"]][0], all_cams[i, 1, :3, :3], all_cams[i, 0], all_maps[i, 0], images[recs[i]["name"]][1])
           for i in mine] if images is not None else None
    if cloud is not None:
        write_cloud_of(out, cloud, rank, world_size, device=all_maps.device, timings=timings)
    built_mesh = None
    refine_views = None
    if refine is not None:
        refine_views = gather_refine_views([(v[0], v[4]) for v in own], all_maps, all_cams, n, rank, world_size, partition)
    if mesh is not None and rank == 0:
        built_mesh = write_mesh_of(all_maps, all_cams, mesh, timings=timings, refine_views=refine_views)
    if dsm is not None:
        if dsm.get("source", "pc") == "mesh":
            built = write_mesh_dsm_of(built_mesh, dsm, device=all_maps.device, timings=timings) if rank == 0 else None
        else:
            built = write_dsm_of(out, dsm, rank, world_size, xyz_device=all_maps.device, timings=timings)
        if ortho is not None:
            write_ortho_of(built[0] if built is not None else None, dsm, ortho, own, rank, world_size, device=all_maps.device,
                           timings=timings)
        if dtm is not None and rank == 0:
            terrain = write_dtm_of(built[0], dsm, dtm, timings=timings)
            if objects is not None:
                write_objects_of(terrain[2], dsm, objects, timings=timings)
    if texture is not None:
        ids = {}
        for per in _gather_objects({i: images[recs[i]["name"]][0] for i in mine}, world_size):
            ids.update(per)
        cameras = [(ids[i], all_cams[i, 1, :3, :3], all_cams[i, 0], W, H) for i in range(n)]
        write_texture_of(built_mesh, texture, own, cameras, rank, world_size, device=all_maps.device, timings=timings)
    return out


def dsm_grid(dsm_settings):
    """(grid, nodata) of a dsm settings dict: the raster every product on the DSM is written on and the value of its empty cells."""
    return (_dsm.DsmGrid(dsm_settings["border"], dsm_settings.get("unit") or (0.1, 0.1), dsm_settings.get("size")),
            dsm_settings.get("nodata", -9999.0))


def gather_refine_views(own, all_maps, all_cams, n_views, rank=0, world_size=1, partition="block"):
    """Every view with its image on rank 0, for the refinement of the mesh that lives there: [(id, K, E, depth [H,W], image)] by
    global view index on rank 0, None elsewhere.  own: this rank's [(id, image [H,W,3] uint8)] in shard order.  Every rank must
    call it.  The images travel in one gather (sharding.gather_points: a row per view, the id in eight trailing bytes); the depth
    maps and cameras are already everywhere.  Rank 0 then refines alone, so the refined mesh is the same bytes for any number of
    ranks."""
    H, W = int(all_maps.shape[2]), int(all_maps.shape[3])
    dev = all_maps.device
    rows = torch.empty((len(own), H * W * 3 + 8), dtype=torch.uint8, device=dev)
    for j, (vid, image) in enumerate(own):
        if tuple(image.shape) != (H, W, 3) or image.dtype != torch.uint8:
            raise ValueError("the refinement needs [%d,%d,3] uint8 reference images (got %s %s)" % (H, W, tuple(image.shape), image.dtype))
        rows[j, :H * W * 3] = image.to(dev).reshape(-1)
        rows[j, H * W * 3:] = torch.tensor([int(vid)], dtype=torch.int64).view(torch.uint8).to(dev)
    rows = sharding.gather_points(rows, rank, world_size)
    if rank != 0:
        return None
    order = [i for r in range(world_size) for i in sharding.shard_views(n_views, r, world_size, partition)]
    views = [None] * n_views
    for j, i in enumerate(order):
        vid = int(rows[j, H * W * 3:].cpu().view(torch.int64)[0])
        views[i] = (vid, all_cams[i, 1, :3, :3], all_cams[i, 0], all_maps[i, 0], rows[j, :H * W * 3].reshape(H, W, 3).contiguous())
    return views


def write_mesh_of(all_maps, all_cams, settings, timings=None, refine_views=None):
    """The mesh of every view (all_maps [n,2,H,W] depth and confidence, all_cams [n,2,4,4], by global view index), written to
    settings["path"] on rank 0; the other ranks do nothing (no collective: the file does not depend on the number of ranks).
    Returns (vertices, faces) as written: the DSM from the mesh and the texture use that mesh.  timings gets mesh_s.
    settings: {"path", "border", "voxel", "trunc", "min_views", "conf_threshold", "views_per_batch"} and optionally the clean steps
    {"min_faces", "spurious", "smooth", "smooth_lambda"}, the hole closing {"close_holes": the longest boundary loop closed, 3 ..
    1024, between the removal and the smoothing} and the decimation {"decimate", "target_faces", "decimate_max_rounds"} (absent:
    off) (mesh.settings_from_args).  mesh.build_and_write builds the mesh of every gathered depth and confidence map with its
    camera, in global view order, and runs the edit steps that are on, in mesh.EDIT_STEPS' order, each on the mesh the one before
    it left and each alone on rank 0, so the file never depends on the number of ranks:
    the clean steps (mesh.clean) and the decimation (mesh.decimate);
    with settings["collapse"] ({"min_edge", "max_edge", "rounds", "depth_tolerance"}; absent: off) the edges the views cannot resolve
    are collapsed (collapse.collapse), against the depth maps and cameras rank 0 already holds, without an image: timings gets
    mesh_collapse_s, a part of mesh_s;
    with settings["flip"] ({"max_angle", "rounds"}; absent: off) the edges are flipped whose flip removes a cap triangle
    (flip.flip_edges): no view, no image and no collective; timings gets mesh_flip_s, a part of mesh_s;
    with settings["subdivide"] ({"max_edge", "rounds", "depth_tolerance"}; absent: off) the mesh is subdivided against the depth
    maps and cameras (subdivide.subdivide): no image and no collective; timings gets mesh_subdivide_s, a part of mesh_s.
    With settings["refine"] (refine.check_refine_settings: {"step", ...}; absent: off) rank 0 then refines the mesh against every
    view's reference image before it writes the PLY (refine.refine_mesh): refine_views is gather_refine_views' list, the other
    ranks' images having reached rank 0 in that one gather; timings gets mesh_refine_s, a part of mesh_s.  The refinement, the DSM
    from the mesh and the texture see the mesh the edit steps left."""
    with timed(timings, "mesh_s"):
        views = [_mesh.MeshView(all_cams[i, 1, :3, :3], all_cams[i, 0], all_maps[i, 0], all_maps[i, 1]) for i in range(all_maps.shape[0])]
        refine = None
        if settings.get("refine") is not None:
            if refine_views is None:
                raise ValueError("the mesh settings ask for a refinement: it needs the views' images (gather_refine_views)")
            rs = _refine.check_refine_settings(settings["refine"])
            ov = [_ortho.OrthoView(i, K, E, d, im) for i, K, E, d, im in refine_views]

            def refine(v, f):
                with timed(timings, "mesh_refine_s", start=True):
                    return _refine.refine_mesh(v, f, ov, **rs)[0]
        res = _mesh.build_and_write(views, settings, refine=refine, timings=timings)
    return res


def write_ortho_of(height, dsm_settings, settings, views, rank=0, world_size=1, device="cuda", timings=None):
    """The true orthophoto on the DSM `height` (rank 0's raster; None elsewhere) of every rank's views, written by rank 0
    (ortho.write_ortho).  views: this rank's [(id, K, E, depth [H,W], image)].  Every rank must call it.
    Rank 0 broadcasts the raster; each rank selects over its own views (ortho.select_views); one all_reduce(MIN) of the keys;
    each rank colours its own winners; one all_reduce(SUM) of the packed RGBA raster and of id + 1 (0 where the rank has no
    winner: one rank contributes per cell).  The exchange is O(raster) whatever the number of views.
    settings: {"path", "depth_tolerance", "views_per_batch"}; the views carry the gathered depth maps, the cameras and the reference
    images.  timings gets ortho_s.  Returns (rgba, view, key) on rank 0, None elsewhere."""
    with timed(timings, "ortho_s"):
        grid = dsm_grid(dsm_settings)[0]
        if rank == 0:
            h = height.to(device=device, dtype=torch.float32).contiguous()
        else:
            h = torch.empty(grid.shape, dtype=torch.float32, device=device)
        if world_size > 1:
            sharding.broadcast_raster(h, 0)
        ov = [_ortho.OrthoView(i, K, E, d, im) for i, K, E, d, im in views]
        tol = settings.get("depth_tolerance", _ortho.DEFAULT_TOLERANCE)
        vpb = settings.get("views_per_batch")
        key = _ortho.select_views(h, grid, ov, tol, views_per_batch=vpb)
        if world_size > 1:
            sharding.all_reduce_raster(key, dist.ReduceOp.MIN)
        rgba, view = _ortho.colorize(key, h, grid, ov, views_per_batch=vpb)
        if world_size > 1:
            both = torch.stack([rgba.view(torch.int32)[:, :, 0], view + 1])
            sharding.all_reduce_raster(both, dist.ReduceOp.SUM)
            rgba = both[0].contiguous().view(torch.uint8).reshape(grid.height, grid.width, 4)
            view = both[1] - 1
        res = None
        if rank == 0:
            _ortho.write_ortho(settings["path"], rgba, grid)
            res = (rgba, view, key)
    return res


def write_texture_of(built_mesh, settings, views, cameras, rank=0, world_size=1, device="cuda", timings=None):
    """The mesh rank 0 built ((vertices, faces); None elsewhere) textured from every rank's views, written by rank 0
    (texture.write_textured_ply).  views: this rank's [(id, K, E, depth [H,W], image)]; cameras: every view's
    (id, K, E, W, H).  Every rank must call it.
    Rank 0 broadcasts the mesh (sizes first); each rank selects over its own views (texture.select_faces); one all_reduce(MIN)
    of the keys; rank 0 lays out the charts, rects and pages (texture.layout) and broadcasts the chart table and page heights;
    each rank fills the charts of its own views; one all_reduce(SUM) of the pages as packed int32 texels (one rank contributes
    per texel); with settings["level"] rank 0 levels the seams of the merged pages (texture.level_pages), with settings["local"]
    it then levels them locally (texture.local_pages); then the empty
    colour.  With settings["smooth_views"] the selection and its all_reduce give way to the candidate lists: each rank builds
    its own (texture.face_candidates), ranks 1.. hand theirs to rank 0 one at a time, merged as they arrive
    (sharding.fold_on with texture.merge_candidates: at most two lists are resident, 128 bytes per face each), and rank 0 smooths
    (texture.smooth_views) and lays out; the other ranks need no keys.  The result then has "label" and "smooth".
    With settings["outliers"] the candidate lists are folded onto rank 0 in the same way; rank 0 broadcasts the merged list
    (sharding.broadcast_raster: one collective of 128 bytes per face); every rank computes the colours of the faces in its own
    views (texture.face_colors); one all_reduce(SUM) of the colour words merges them (a slot belongs to one view, so to one rank,
    and the others hold 0 there); rank 0 rejects in place (texture.reject_outliers), then smooths or takes column 0, and lays
    out.  The result then has "rejected" and "outliers".
    With settings["ortho"] ({"path", "border", "unit", "size", "z_down"}; absent or None: off) rank 0 renders the orthophoto of the
    textured mesh after the texcoords, top-down from the atlas, the mesh and the texcoords it holds (ortho_mesh.build_and_write), and
    writes the RGBA .tif and .tfw: no new collective, so the file does not depend on the number of ranks; the result then has
    "ortho" (ortho_mesh.summary's dict) and timings gets texture_ortho_s (a part of texture_s).
    settings: {"path", "depth_tolerance", "views_per_batch", "page_size", "pad", and optionally "level" (None, or the seam
    levelling's settings), "local" (the local seam levelling's), "smooth_views", "outliers" and "ortho"} (texture.settings_from_args);
    the mesh is the one rank 0 wrote, after its edit steps; rank 0 writes the textured PLY and its pages; timings gets texture_s.
    Returns texture.texture_mesh's dict on rank 0 (without "labels"), None elsewhere."""
    with timed(timings, "texture_s"):
        tol, vpb, P, pad = _tx.check_settings(settings)
        level = _tx.check_level_settings(settings["level"]) if settings.get("level") is not None else None
        local = _tx.check_local_settings(settings["local"]) if settings.get("local") is not None else None
        smooth = _tx.check_smooth_settings(settings["smooth_views"]) if settings.get("smooth_views") is not None else None
        outliers = _tx.check_outlier_settings(settings["outliers"]) if settings.get("outliers") is not None else None
        v = f = None
        if rank == 0:
            v = built_mesh[0].to(device=device, dtype=torch.float32).contiguous()
            f = built_mesh[1].to(device=device, dtype=torch.int32).contiguous()
        v = sharding.broadcast_rows(v, (3,), torch.float32, device)
        f = sharding.broadcast_rows(f, (3,), torch.int32, device)
        ov = [_ortho.OrthoView(i, K, E, d, im) for i, K, E, d, im in views]
        smoothed = {}
        if smooth is None and outliers is None:
            key = _tx.select_faces(v, f, ov, tol, views_per_batch=vpb)
            if world_size > 1:
                sharding.all_reduce_raster(key, dist.ReduceOp.MIN)
        else:
            cand = sharding.fold_on(_tx.face_candidates(v, f, ov, tol, views_per_batch=vpb), _tx.merge_candidates)
            if outliers is not None:
                if cand is None:
                    cand = torch.empty((int(f.shape[0]), _tx.CANDIDATES), dtype=torch.int64, device=device)
                sharding.broadcast_raster(cand, 0)
                col = sharding.all_reduce_raster(_tx.face_colors(v, f, cand, ov, views_per_batch=vpb), dist.ReduceOp.SUM)
                if rank == 0:
                    cand, rejected, counts = _tx.reject_outliers(cand, col, outliers, out=cand)
                    smoothed = {"rejected": rejected, "outliers": _tx.outlier_summary(counts, outliers, cand.shape[0])}
                del col
            if rank == 0 and smooth is not None:
                key, label, commits = _tx.smooth_views(f, int(v.shape[0]), cand, *smooth)
                before = _tx.charts(f, cand[:, 0].contiguous(), int(v.shape[0]))[1]
                smoothed.update({"label": label, "smooth": _tx.smooth_summary(cand, label, commits, smooth[2], before.shape[0])})
            elif rank == 0:
                key = cand[:, 0].contiguous()
            del cand
        res = None
        table = heights = None
        if rank == 0:
            cams = [_tx.Camera(*c) for c in cameras]
            chart, _, rects, packing, table_np = _tx.layout(v, f, key, cams, P, pad)
            table = torch.from_numpy(table_np).to(device)
            heights = torch.tensor(packing.heights, dtype=torch.int64, device=device)
            res = dict(smoothed, key=key, chart=chart, rects=rects, packing=packing, table=table_np)
        table = sharding.broadcast_rows(table, (8,), torch.int32, device)
        heights = sharding.broadcast_rows(heights, (), torch.int64, device)
        table_np = table.cpu().numpy()
        packing = res["packing"] if rank == 0 else _tx.Packing(table_np[:, [6, 4, 5]].astype(np.int64), heights.cpu().tolist(), P)
        atlas = _tx.fill_pages(table_np, packing, ov, _tx.new_atlas(packing, device))
        if world_size > 1:
            sharding.all_reduce_raster(atlas, dist.ReduceOp.SUM)
        keep = {}   # what the local step reuses of the global one
        if level is not None and rank == 0:   # the merged atlas, the mesh, keys, table and every camera are here: no new collective
            res["level"] = _tx.level_pages(v, f, key, res["chart"], table_np, packing, cams, atlas, *level,
                                           keep=keep if local is not None else None)
        if local is not None and rank == 0:   # right after the global step, on the same atlas: no new collective either
            res["local"] = _tx.local_pages(v, f, key, res["chart"], table_np, packing, cams, atlas, *local, cover=keep.get("cover"),
                                           pairs=keep.get("pairs"))
        del keep
        _tx.finish_pages(atlas)
        if rank == 0:
            tc, tn = _tx.texcoords(v, f, key, res["chart"], table_np, packing, cams)
            res.update(pages=_tx.split_pages(atlas, packing), texcoord=tc, texnumber=tn)
            _tx.write_textured_ply(settings["path"], v, f, tc, tn, res["pages"])
            if settings.get("ortho") is not None:   # the finished atlas, the mesh and the texcoords are here: no new collective
                with timed(timings, "texture_ortho_s", start=True):
                    page_row = torch.from_numpy(packing.page_row).to(device)
                    res["ortho"] = _om.build_and_write(v, f, tc, tn, atlas, page_row, settings["ortho"])[2]
    return res


def reference_colors(image, H, W):
    """A reference crop (device uint8 [H,W,C], C = 1 or 3, predict.reference_crop) as extract_points' ref_img: [H,W,3] float32,
    byte / 255, a grey crop repeated to three channels.  int(c * 255.0f) in the gather kernel returns every byte exactly."""
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] not in (1, 3):
        raise ValueError("the cloud needs [H,W,1] or [H,W,3] uint8 reference crops (got %s %s)" % (tuple(image.shape), image.dtype))
    if tuple(image.shape[:2]) != (H, W):
        raise ValueError("a reference crop of %d x %d on maps of %d x %d: the cloud's colours need them equal"
                         % (image.shape[0], image.shape[1], H, W))
    if image.shape[2] == 1:
        image = image.expand(H, W, 3)
    return (image.to(torch.float32) / 255.0).contiguous()


def write_cloud_of(results, settings, rank=0, world_size=1, device="cuda", timings=None):
    """The merged cloud of the points of `results` (predict_and_fuse's list, with colours) over all ranks, written by rank 0
    (cloud.build_and_write).  Every rank must call it: one gather_points of [n, 9] int32 rows (the int32 colours, and xyz and the
    normals bit-cast: no arithmetic touches them on the way).  Returns (cloud dict, summary) on rank 0, None elsewhere.
    settings: {"path", "border", "voxel", "min_points"} (cloud.check_settings).  Every reference view's crop colours its points
    (extract_points' ref_img, the bytes / 255; a grey crop repeated to three channels; a crop of another size than the map is
    refused: reference_colors); without the cloud points["color"] stays None.  Each rank concatenates the xyz, normal and colour of
    its results, the gather moves them to rank 0, and rank 0 merges them on the voxel grid and writes the PLY; timings gets cloud_s.
    With filter_sources=False the file does not depend on the number of ranks.  The crops are the sweeping rank's, so with more than
    one rank fuse_partition must be "views".  With settings["outliers"] ({"radius", "k", "alpha", "min_neighbours"}; absent or None:
    off) rank 0 filters the merged cloud before it writes it (cloud_outliers.filter_cloud, checked up front with the cloud
    settings): no new collective; timings gets cloud_outliers, the filter's info."""
    with timed(timings, "cloud_s"):
        rows = []
        for r in results:
            p = r["points"]
            if p["color"] is None or p["normal"] is None:
                raise ValueError("the cloud needs the colours and normals of every result (%s has none)" % r["ref"])
            rows.append(torch.cat([p["xyz"].view(torch.int32), p["normal"].view(torch.int32), p["color"]], 1))
        local = torch.cat(rows) if rows else torch.zeros((0, 9), dtype=torch.int32, device=device)
        pts = sharding.gather_points(local.contiguous(), rank, world_size)
        res = None
        if rank == 0:
            res = _cloud.build_and_write(pts[:, 0:3].contiguous().view(torch.float32), pts[:, 3:6].contiguous().view(torch.float32),
                                         pts[:, 6:9].contiguous(), settings)
    if timings is not None and res is not None and "outliers" in res[1]:
        timings["cloud_outliers"] = res[1]["outliers"]   # the filter's info, for the caller's report
    return res


def write_dsm_of(results, settings, rank=0, world_size=1, xyz_device="cuda", timings=None):
    """The DSM of the points of `results` (predict_and_fuse's list) over all ranks, written by rank 0 (dsm.build_and_write).
    Every rank must call it.  Returns (height, count) on rank 0, None elsewhere.
    settings: {"path", "border", "unit", "size", "select", "trim", "min_points", "interpolation", "radius", "iterations", "nodata"}
    (dsm.build_and_write), without "source" or with "source": "pc".  The xyz of every result of this rank are concatenated, gathered
    on rank 0 (sharding.gather_points) and the DSM is built and written there; timings gets dsm_s."""
    with timed(timings, "dsm_s"):
        parts = [r["points"]["xyz"] for r in results]
        local = torch.cat(parts) if parts else torch.zeros((0, 3), dtype=torch.float32, device=xyz_device)
        pts = sharding.gather_points(local.to(torch.float32).contiguous(), rank, world_size)
        res = _dsm.build_and_write(pts, settings, device=local.device) if rank == 0 else None
    return res


def write_mesh_dsm_of(built_mesh, settings, device="cuda", timings=None):
    """Rank 0's DSM of the mesh write_mesh_of returned ((vertices, faces)), written there (dsm.build_and_write_mesh).
    Returns (height, None): the shape of write_dsm_of's result, with no point count.
    settings: write_dsm_of's with "source": "mesh" (needs the mesh; select Max, min_points 1: dsm.check_mesh_settings).  No point
    is gathered and there is no collective, so the file does not depend on the number of ranks; timings gets dsm_s on rank 0."""
    with timed(timings, "dsm_s"):
        vertices, faces = built_mesh
        h = _dsm.build_and_write_mesh(vertices, faces, settings, device=device)
    return h, None


def write_dtm_of(height, dsm_settings, settings, timings=None):
    """Rank 0's DTM of the height raster the DSM step returned, on the DSM's grid and with its nodata (dtm.build_and_write);
    no collective.  Returns (dtm, level, ndsm).
    settings: {"path", "ndsm", "ground", "max_window", "slope", "dh0", "dh_max"} (dtm.check_settings).  The raster is the DSM's of
    either source, after any MovingAverage fill, which is part of the DSM; rank 0 writes the DTM and, when asked, the nDSM and the
    level raster; timings gets dtm_s on rank 0."""
    with timed(timings, "dtm_s"):
        grid, nodata = dsm_grid(dsm_settings)
        res = _dtm.build_and_write(height, grid, dict(settings, nodata=nodata))
    return res


def write_objects_of(ndsm, dsm_settings, settings, timings=None):
    """Rank 0's objects of the nDSM the DTM step returned, on the DSM's grid and with its nodata (objects.build_and_write); no
    collective.  Returns (label, table).
    settings: {"path", "table", "min_height", "min_area", "connectivity", "open", "outlines"} (objects.check_settings).  Rank 0
    writes the label raster and, when asked, the table and the outlines; timings gets objects_s on rank 0, and objects_outlines_s
    (a part of it) when the outlines are on."""
    with timed(timings, "objects_s"):
        grid, nodata = dsm_grid(dsm_settings)
        res = _objects.build_and_write(ndsm, grid, dict(settings, nodata=nodata), timings=timings)
    return res


def add_estimated_normals(views, pairs, fusion_num=10, nei=1):
    """Sets views[name]["normal"] (ops.normals_from_depth of views[name]["depth"] with views[name]["K"]) for every view that
    fuse.fuse_block(views, pairs, fusion_num=...) reads -- each reference view and its first fusion_num listed sources that
    exist -- and has none yet.  Call it before fuse_block: the source-filtering chain then never reaches the normals.
    These are what the reference's fusion reads from {view}_normal.pfm (fusion_3d_normal.py:437-443, 491-498).  predict_and_fuse
    computes them after the all-gather (the exchange is unchanged), from the unfiltered gathered maps (the reference reads them from
    depth_path, not from its tmp folder), once per view this rank's fusion touches; normals follow the view, so the fused arrays do
    not depend on the number of ranks any more than without them."""
    from . import ops

    for pair in pairs:
        for name in [pair["ref"]] + [n for n in pair["src"][:fusion_num] if n in views]:
            v = views[name]
            if v.get("normal") is None:
                v["normal"] = ops.normals_from_depth(v["depth"], v["K"], nei=nei)
    return views


def save_fused(results, folder):
    """One <folder>/<ref>.npz per reference view: final_mask (bit-packed rows), xyz [n,3], normal [n,3], views [n,n_vis] (sorted
    0-based image indices, -1 padded), nviews [n].  The OpenMVS .mvs / .ply writers (IO/mvs_io.py) are out of scope:
    these arrays are what Interface_Fused would be handed (fusion_3d_normal.py:558-570)."""
    os.makedirs(folder, exist_ok=True)
    paths = []
    for r in results:
        p = r["points"]
        sub = os.path.join(folder, "scene_%d" % r["scene"]) if "scene" in r else folder   # (a view can belong to several scene blocks)
        os.makedirs(sub, exist_ok=True)
        path = os.path.join(sub, r["ref"] + ".npz")
        fm = r["final_mask"].cpu().numpy()
        np.savez(path, mask_shape=np.array(fm.shape), final_mask=np.packbits(fm, axis=1), xyz=p["xyz"].cpu().numpy(),
                 normal=p["normal"].cpu().numpy() if p["normal"] is not None else np.zeros((0, 3), np.float32),
                 views=p["views"].cpu().numpy(), nviews=p["nviews"].cpu().numpy(), n_valid=np.array(p["n_valid"]))
        paths.append(path)
    return paths
