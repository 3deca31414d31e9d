#!/usr/bin/env python3
"""Register budget of the hand-scheduled kernels (csrc: the parts of vrt_device.hip, vrt_denoise.hip over its vrt_denoise_*.h, vrt_scene_edit.hip, vrt_scene_read.hip, vrt_brush.hip, vrt_flood.hip, vrt_voxelize.hip, vrt_morph.hip, vrt_components.hip, vrt_query.hip, vrt_query_seg.hip, vrt_reproject.hip, vrt_reproject_cam.hip, vrt_upsample.hip, vrt_upsample_cam.hip, vrt_rays.hip, vrt_render_rays.hip), checked
at build time.

K1's look-up loop pins physical registers and the kernel sits at two occupancy cliffs that the compiler's own remark does
not show: past 80 scalar registers a SIMD holds seven of these waves, not eight (measured: DESIGN.md 5, "Tile tags"), and
past 64 vector registers likewise.  `make -C voxel-raytracing_amd/csrc resources` (and tests/test_kernel_resources.py)
compile these objects (side by side, four at a time) with -Rpass-analysis=kernel-resource-usage and fail when a product kernel leaves its budget: one more
live scalar then breaks the build instead of silently costing 7 %.
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voxel-raytracing_amd", "csrc")

# mangled-name fragment -> (what it is, max VGPRs, max SGPRs, max scratch bytes per lane)
BUDGET = {
    "k_primaryILi7ELb0ELi1ELb0ELi0EE": ("K1 primary-only, look-up loop, one frame per launch (rows dealt to the XCDs)", 64, 80, 0),
    "k_primaryILi7ELb0ELi1ELb0ELi2EE": ("K1 primary-only, look-up loop, 8 frames in the kernel arguments (XCD regions)", 64, 80, 0),
    "k_primaryILi7ELb0ELi1ELb1ELi0EE": ("K1 primary-only, look-up loop, slots in the table, rows dealt to the XCDs (the bench line's kernel)", 64, 80, 0),
    "k_primaryILi7ELb0ELi1ELb1ELi2EE": ("K1 primary-only, look-up loop, slots in the table, XCD regions", 64, 80, 0),
    # (round 4: with the AO rays' pool the kernel needs 65 VGPRs, i.e. 7 waves per SIMD; forced into 64 it spills 12 B per lane and runs
    # the same 124-128 us on the reference defaults: tools/exp_r4_breakdown.py, libvrt_hip_m8.so -- no scratch is the invariant kept)
    "k_primaryILi7ELb0ELi4ELb0ELi0EE": ("megakernel without its bounce loop, one frame per launch", 72, 80, 0),
    "k_primaryILi7ELb0ELi4ELb1ELi2EE": ("megakernel without its bounce loop, table", 72, 96, 0),
    "k_primaryILi7ELb0ELi2ELb0ELi0EE": ("megakernel with the stack of hits (context option packed_bounces = 0), one frame per launch", 72, 96, 512),
    "k_primaryILi7ELb0ELi2ELb1ELi2EE": ("megakernel with the stack of hits, table", 72, 96, 512),
    "k_primaryILi7ELb0ELi5ELb0ELi0EE": ("megakernel, bounce chain as one word per hit, <= 2 bounces (BASELINE configs[3]), one frame per launch", 72, 96, 160),
    "k_primaryILi7ELb0ELi6ELb0ELi0EE": ("megakernel, bounce chain as one word per hit, <= 5 bounces (the reference's defaults), one frame per launch", 72, 96, 192),
    "k_primaryILi6ELb0ELi2ELb0ELi0EE": ("megakernel over bricks (config 5), one frame per launch", 80, 96, 576),
    "k_denoise_ldsILb0ELb0ELb0ELb1EE": ("K3 weighted pass, exact, packed", 128, 96, 0),
    # (the verified pass: four workgroups of four waves per compute unit, i.e. at most 128 VGPRs; 96 leaves it five)
    "k_denoise_verILb0ELb1ELi3ELb0EE": ("K3 verified weighted pass, tap offset 3 (the reference's pass 1)", 96, 96, 0),
    "k_denoise_verILb0ELb1ELi5ELb0EE": ("K3 verified weighted pass, tap offset 5 (the reference's pass 2)", 96, 96, 0),
    "k_denoise_verILb0ELb1ELi1ELb1EE": ("K3 verified pass 0", 64, 96, 0),
    # (round 4, every weight computed once: R waves per workgroup, five to six workgroups per compute unit by LDS: 96 VGPRs leave five waves per SIMD)
    "k_denoise_pairILb1ELi3EE": ("K3 verified weighted pass, every weight once, tap offset 3 (the reference's pass 1)", 96, 96, 0),
    "k_denoise_pairILb1ELi5EE": ("K3 verified weighted pass, every weight once, tap offset 5 (the reference's pass 2)", 96, 96, 0),
    "k_denoise_pairILb0ELi3EE": ("K3 VRT_DENOISE_FAST weighted pass, every weight once, tap offset 3", 96, 96, 0),
    "k_denoise_p0ILb1EE": ("K3 verified pass 0, a wave to itself (no LDS ring, no barrier)", 64, 96, 0),
    # the numeric spec's primitives one per element (vrt_debug_spec, vrt_device.hip part 0): a diagnostic, no cliff to guard; no spill
    "k_debug_specEjPKjS1_S1_mPj": ("diagnostic: one primitive of vrt_spec.h per element", 32, 48, 0),
    # scene edits (vrt_scene_edit_box): no register cliff to guard, but none of them may spill
    "k_edit_writeEPhS0_": ("scene edit: the box's ids into the volume and field 8", 64, 96, 0),
    "k_edit_occ1EPKh": ("scene edit: occ1 words under the box", 64, 96, 0),
    "k_edit_occ_upEPKm": ("scene edit: occ2 / occ3 words under the box", 64, 96, 0),
    "k_edit_pass_xENS_9EditPassXE": ("scene edit: clearance pass x, ballot and carry", 64, 96, 0),
    "k_edit_pass_ldsENS_9EditPassLE": ("scene edit: clearance passes y and z on LDS", 64, 96, 0),
    "k_edit_open_scanENS_8EditOpenEi": ("scene edit: open-cell scans along y and z within Q_o", 64, 96, 0),
    "k_edit_open_xENS_8EditOpenE": ("scene edit: open-cell scan along x and the bytes of Q_o", 64, 96, 0),
    "k_bedit_classifyENS_9BrickEditE": ("brick-scene edit: which bricks of T are occupied after the edit", 64, 96, 0),
    "k_bedit_writeENS_9BrickEditE": ("brick-scene edit: the box's ids into the pool bricks of T", 64, 96, 0),
    "k_bedit_extractENS_11BrickCoarseE": ("brick-scene edit: the occupancy of E as a lattice of its own", 64, 96, 0),
    "k_bedit_copyENS_11BrickCoarseE": ("brick-scene edit: R_o into the coarse fields", 64, 96, 0),
    # scene read-back (vrt_scene_read.hip): gathers and a ballot per wave -- no register cliff to guard, none may spill (4 .. 28 VGPRs)
    "k_read_boxILb0EE": ("scene read-back: a box of a dense scene into the staging buffer", 32, 48, 0),
    "k_read_boxILb1EE": ("scene read-back: a box of a brick scene through the packed entries", 32, 48, 0),
    "k_list_bricksENS_7ReadBoxE": ("scene read-back: occupied bricks under a box", 32, 64, 0),
    "k_list_countILb0EE": ("scene read-back: non-empty voxels per segment, dense", 32, 48, 0),
    "k_list_countILb1EE": ("scene read-back: non-empty voxels per segment, bricks", 32, 48, 0),
    "k_list_scanEPjj": ("scene read-back: exclusive scan of the segments' counts", 32, 48, 0),
    "k_list_scatterILb0EE": ("scene read-back: the records to their places, dense", 32, 48, 0),
    "k_list_scatterILb1EE": ("scene read-back: the records to their places, bricks", 32, 48, 0),
    # brushes and stamps (vrt_brush.hip): a gather, integer predicates in 64 bits and a ballot per wave -- no register cliff to guard,
    # none may spill (16 .. 23 VGPRs, 36 .. 50 SGPRs)
    "k_brush_extentILi0EE": ("brush: what a box changes (count, bounds, ids written)", 32, 64, 0),
    "k_brush_extentILi1EE": ("brush: what an ellipsoid changes", 32, 64, 0),
    "k_brush_extentILi2EE": ("brush: what a capsule changes", 32, 64, 0),
    "k_brush_extentILi3EE": ("stamp: what the oriented source box changes", 32, 64, 0),
    "k_brush_composeILi0EE": ("brush: the tight box's new ids into the edit scratch, box", 32, 64, 0),
    "k_brush_composeILi1EE": ("brush: the tight box's new ids, ellipsoid", 32, 64, 0),
    "k_brush_composeILi2EE": ("brush: the tight box's new ids, capsule", 32, 64, 0),
    "k_brush_composeILi3EE": ("stamp: the tight box's new ids", 32, 64, 0),
    # flood fill (vrt_flood.hip): gathers, ballots and a tile relaxed in LDS -- no register cliff to guard, none may spill
    "k_flood_passENS_8FloodJobE": ("flood: the passable mask and the seed's bit", 32, 64, 0),
    "k_flood_roundILi6EE": ("flood: one round over the active tiles, 6-connectivity", 32, 64, 0),
    "k_flood_roundILi26EE": ("flood: one round over the active tiles, 26-connectivity", 32, 64, 0),
    "k_flood_extentENS_8FloodJobE": ("flood: the region and what it changes (counts, bounds)", 32, 64, 0),
    "k_flood_composeENS_8FloodJobE": ("flood: the tight box's new ids into the edit scratch", 32, 64, 0),
    # mesh voxelization (vrt_voxelize.hip): a wave-uniform triangle held in scalar registers (k_vox_surface has the most of them: the
    # triangle, the job and the row's five axes), 64-bit integer tests per lane -- no register cliff to guard, none may spill
    "k_vox_surfaceENS_6VoxJobE": ("voxelize: a triangle's slab of rows, 64 voxels a ballot, into the coverage mask", 32, 112, 0),
    "k_vox_crossENS_6VoxJobE": ("voxelize: a triangle's crossings, one column a lane, into the toggle mask", 32, 96, 0),
    "k_vox_scanENS_6VoxJobE": ("voxelize: the toggle mask's rows scanned into the coverage mask", 32, 64, 0),
    "k_vox_extentENS_6VoxJobE": ("voxelize: the covered count and what changes (counts, bounds)", 32, 64, 0),
    "k_vox_composeENS_6VoxJobE": ("voxelize: the tight box's new ids into the edit scratch", 32, 64, 0),
    # morphology (vrt_morph.hip): gathers, ballots and a tile stepped r times in LDS (32 KiB a workgroup) -- no register cliff to
    # guard, none may spill (16 .. 22 VGPRs, 36 .. 46 SGPRs)
    "k_morph_passENS_8MorphJobE": ("morphology: the solid mask over the domain", 32, 64, 0),
    "k_morph_stepILi6EE": ("morphology: one phase, r unit steps a tile, 6-connectivity", 32, 64, 0),
    "k_morph_stepILi26EE": ("morphology: one phase, r unit steps a tile, 26-connectivity", 32, 64, 0),
    "k_morph_extentENS_8MorphJobE": ("morphology: what changes (added, removed, bounds)", 32, 64, 0),
    "k_morph_composeENS_8MorphJobE": ("morphology: the tight box's new ids into the edit scratch", 32, 64, 0),
    # connected components (vrt_components.hip): a union-find over the label volume, ballots, 5 KB of LDS in the tile pass -- no register
    # cliff to guard, none may spill (8 .. 44 VGPRs, 16 .. 72 SGPRs)
    "k_comp_tileILi6ELb0EE": ("components: labels inside a tile, 6-connectivity", 64, 80, 0),
    "k_comp_tileILi6ELb1EE": ("components: labels inside a tile, 6-connectivity, equal ids", 64, 80, 0),
    "k_comp_tileILi26ELb0EE": ("components: labels inside a tile, 26-connectivity", 64, 80, 0),
    "k_comp_tileILi26ELb1EE": ("components: labels inside a tile, 26-connectivity, equal ids", 64, 80, 0),
    "k_comp_seamILi6EE": ("components: unions across tile faces", 32, 64, 0),
    "k_comp_seamILi26EE": ("components: unions across tile faces, edges and corners", 32, 64, 0),
    "k_comp_flattenENS_7CompJobE": ("components: labels to roots, roots counted per segment", 32, 64, 0),
    "k_comp_numberENS_7CompJobE": ("components: roots numbered in order, table entries written", 32, 64, 0),
    "k_comp_measureENS_7CompJobE": ("components: numbers into the labels, counts and boxes per tile", 32, 64, 0),
    "k_comp_summaryENS_7CompJobE": ("components: the largest and the voxel total", 32, 64, 0),
    "k_comp_selectENS_7CompJobE": ("components: the filter's verdict per component", 32, 64, 0),
    "k_comp_extentENS_7CompJobE": ("components: what the filter changes (count, bounds)", 32, 64, 0),
    "k_comp_composeENS_7CompJobE": ("components: the tight box's new ids into the edit scratch", 32, 64, 0),
    "k_comp_labelsENS_7CompJobE": ("components: a box of labels for the host", 32, 64, 0),
    # ray queries (vrt_query.hip): k_query<TRAV, ANYHIT, PICK>; none may spill.  The closest-hit form over the look-up loop keeps the
    # ray's direction and first mapPos across the march for the hit record: seven waves per SIMD, the others eight
    "k_queryILi7ELb0ELb0EE": ("ray query, closest hit, look-up loop", 72, 80, 0),
    "k_queryILi7ELb1ELb0EE": ("ray query, any hit, look-up loop", 64, 80, 0),
    "k_queryILi7ELb0ELb1EE": ("pixel pick, look-up loop", 64, 80, 0),
    "k_queryILi4ELb0ELb0EE": ("ray query, closest hit, DF (volumes past the 32-bit field layout)", 64, 80, 0),
    "k_queryILi4ELb1ELb0EE": ("ray query, any hit, DF", 64, 80, 0),
    "k_queryILi4ELb0ELb1EE": ("pixel pick, DF", 64, 80, 0),
    "k_queryILi6ELb0ELb0EE": ("ray query, closest hit, brick march", 64, 80, 0),
    "k_queryILi6ELb1ELb0EE": ("ray query, any hit, brick march", 64, 80, 0),
    "k_queryILi6ELb0ELb1EE": ("pixel pick, brick march", 64, 80, 0),
    # ray segments (vrt_query_seg.hip): k_query_seg<TRAV, ANYHIT>; none may spill.  Both forms run the closest-hit march and keep the
    # ray's origin, direction and limit across it for t_hit (75 / 69 / 55 VGPRs closest hit, 57 / 61 / 43 any hit): six waves per
    # SIMD for the closest hit over the look-up loop, seven over the bricks, the others eight
    "k_query_segILi7ELb0EE": ("ray segment, closest hit, look-up loop", 80, 80, 0),
    "k_query_segILi7ELb1EE": ("ray segment, any hit, look-up loop", 64, 80, 0),
    "k_query_segILi4ELb0EE": ("ray segment, closest hit, DF", 64, 80, 0),
    "k_query_segILi4ELb1EE": ("ray segment, any hit, DF", 64, 80, 0),
    "k_query_segILi6ELb0EE": ("ray segment, closest hit, brick march", 72, 80, 0),
    "k_query_segILi6ELb1EE": ("ray segment, any hit, brick march", 64, 80, 0),
    # temporal reprojection (vrt_reproject.hip): a streaming kernel with a four-tap gather; eight waves per SIMD, no scratch (40 VGPRs, 58 SGPRs)
    "k_reprojectENS_15ReprojectParamsE": ("temporal reprojection", 64, 80, 0),
    # temporal reprojection for ray cameras (vrt_reproject_cam.hip): k_reproject's memory side, one instantiation per camera model
    # (40 VGPRs each; 58 / 50 / 48 SGPRs); eight waves per SIMD, no scratch, no LDS
    "k_reproject_camILi0EE": ("temporal reprojection, perspective camera", 64, 80, 0),
    "k_reproject_camILi1EE": ("temporal reprojection, orthographic camera", 64, 80, 0),
    "k_reproject_camILi2EE": ("temporal reprojection, panorama", 64, 80, 0),
    # temporal upsampling (vrt_upsample.hip): one thread per display pixel, two projections and the same four-tap gather; eight
    # waves per SIMD, no scratch (40 VGPRs, 62 SGPRs)
    "k_upsampleENS_14UpsampleParamsE": ("temporal upsampling", 64, 80, 0),
    # temporal upsampling for ray cameras (vrt_upsample_cam.hip): k_upsample's memory side, one instantiation per camera model
    # (40 / 40 / 42 VGPRs; 62 / 62 / 52 SGPRs); eight waves per SIMD, no scratch, no LDS
    "k_upsample_camILi0EE": ("temporal upsampling, perspective camera", 64, 80, 0),
    "k_upsample_camILi1EE": ("temporal upsampling, orthographic camera", 64, 80, 0),
    "k_upsample_camILi2EE": ("temporal upsampling, panorama", 64, 80, 0),
    # ray generation for caller-side cameras (vrt_rays.hip): a stream of 24 B per pixel; eight waves per SIMD, no scratch (15 VGPRs, 35 / 36 SGPRs)
    "k_camera_raysENS_12RayCamConstsE": ("ray generation, three camera models", 32, 48, 0),
    "k_camera_rays_offsetENS_12RayCamConstsE": ("ray generation with a sub-pixel offset, three camera models", 32, 48, 0),
    # the G-buffer of caller-supplied rays (vrt_render_rays.hip).  k_rays_primary<TRAV> is k_query's closest-hit form plus the plane
    # stores: the same budgets, no scratch (69 / 48 / 59 VGPRs).  k_shade_rays<TRAV> is k_shade's body: four waves per SIMD (at most 128
    # VGPRs; 108 / 89 / 108) and k_shade's 368 B of scratch per lane, the stack of hits of the bounce loop -- nothing beyond it
    "k_rays_primaryILi7EE": ("rays' G-buffer, primary march, look-up loop", 72, 80, 0),
    "k_rays_primaryILi4EE": ("rays' G-buffer, primary march, DF", 64, 80, 0),
    "k_rays_primaryILi6EE": ("rays' G-buffer, primary march, brick march", 64, 80, 0),
    "k_shade_raysILi7EE": ("rays' G-buffer, shading of the hit list, look-up loop", 128, 112, 368),
    "k_shade_raysILi4EE": ("rays' G-buffer, shading of the hit list, DF", 128, 112, 368),
    "k_shade_raysILi6EE": ("rays' G-buffer, shading of the hit list, brick march", 128, 112, 368),
}


# the objects that hold budgeted kernels, as the Makefile builds them: (source, extra flags); slowest first
OBJECTS = [("vrt_device.hip", ["-DVRT_K1_PART=%d" % n]) for n in (3, 0, 1, 2)] + [("vrt_denoise.hip", []), ("vrt_scene_edit.hip", []), ("vrt_scene_read.hip", []), ("vrt_brush.hip", []), ("vrt_flood.hip", []), ("vrt_voxelize.hip", []), ("vrt_morph.hip", []), ("vrt_components.hip", []), ("vrt_query.hip", []), ("vrt_query_seg.hip", []),
                                                                                     ("vrt_reproject.hip", []), ("vrt_reproject_cam.hip", []), ("vrt_upsample.hip", []), ("vrt_upsample_cam.hip", []), ("vrt_rays.hip", []),
                                                                                     ("vrt_render_rays.hip", [])]


def remarks(obj):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
             "-fhip-fp32-correctly-rounded-divide-sqrt", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value", "-Wno-pass-failed",
             "-Rpass-analysis=kernel-resource-usage", "-c", "-o", "/dev/null"]
    p = subprocess.run([hipcc] + flags + obj[1] + [obj[0]], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if p.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + p.stdout[-4000:])
    return p.stdout


def report():
    with ThreadPoolExecutor(max_workers=4) as pool:                  # four compiler processes at a time
        out = "\n".join(pool.map(remarks, OBJECTS))
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" ")[0]] = int(m.group(2))
    return kernels


def check(kernels=None):
    kernels = kernels if kernels is not None else report()
    bad, rows = [], []
    for frag, (what, vmax, smax, scr) in BUDGET.items():
        hits = [(n, k) for n, k in kernels.items() if frag in n]
        if not hits:
            bad.append(f"{frag}: kernel not found in the resource report ({what})")
            continue
        for n, k in hits:
            rows.append((frag, k.get("VGPRs"), k.get("TotalSGPRs"), k.get("ScratchSize"), what))
            if k.get("VGPRs", 1 << 30) > vmax: bad.append(f"{frag}: {k.get('VGPRs')} VGPRs > {vmax} ({what})")
            if k.get("TotalSGPRs", 1 << 30) > smax: bad.append(f"{frag}: {k.get('TotalSGPRs')} SGPRs > {smax} ({what})")
            if k.get("ScratchSize", 1 << 30) > scr: bad.append(f"{frag}: {k.get('ScratchSize')} B scratch per lane > {scr} ({what})")
    return bad, rows


if __name__ == "__main__":
    bad, rows = check()
    for frag, v, s, sc, what in rows:
        print(f"{frag:36s} VGPR {v:3d}  SGPR {s:3d}  scratch {sc:4d}   {what}")
    if bad:
        print("\nregister budget exceeded:\n  " + "\n  ".join(bad), file=sys.stderr)
        sys.exit(1)
    print("register budgets hold")
