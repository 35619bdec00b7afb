"""Regenerate include/d3h.h from the extern "C" definitions in d3human-code_amd/csrc/*.hip (signatures + their leading comments),
grouped per source file with the reference interface each group replaces, and d3human-code_amd/d3h/_abi.py, the same signatures as
a table the ctypes binding (d3h/_lib.py) sets argtypes from and checks every call against."""
import glob, os, re
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = {
    'sdf_mlp.hip': 'SDF query, forward: geometry/embedding.py:21-38 (Embedding.forward) + geometry/mlp.py:34-45 (MLP.forward) + geometry/hmsdf.py:433-444 (v_deformed, chunked sweep)',
    'sdf_mlp_x3.hip': 'SDF query, forward, on the bf16 matrix pipe at fp32 accuracy (three-way operand split): the same reference functions as sdf_mlp.hip',
    'sdf_mlp_bwd.hip': 'SDF query, backward: autograd of geometry/mlp.py:34-45 as run by loss.backward() (train.py:742); eikonal term geometry/hmsdf.py:856-876 (autograd.grad(..., create_graph=True) + its backward)',
    'marching_tets.hip': 'G-Shell marching tetrahedra: geometry/gshell_tets.py:253-447 (GShell_Tets.__call__), geometry/hmsdf_tets_split.py:254-454 (hmSDF_Tets.__call__); static edge list geometry/hmsdf.py:382-388',
    'lbs.hip': 'SMPL-X skinning of surface points: deform/smplx_exavatar_deformer.py:363-383 (interpolate_weights -> pytorch3d knn_points with K = self.k, 1..32, third_parties/pytorch3d/cuda/knn.cu:205, knn_cpu.cpp:13-128), :385-421 (apply_lbs_inverse), :434-486 (lbs_forward)',
    'smplx_pose.hip': 'SMPL-X pose -> joint transforms: deform/smplx_exavatar/lbs.py:311-347 (batch_rodrigues), :361-413 (batch_rigid_transform) as used by lbs() :216-247 from deform/smplx_exavatar/body_models.py:1225-1257',
    'raster.hip': 'nvdiffrast replacements (un-vendored; call sites render/render.py:37 interpolate, :72,:102 texture, :381 antialias, :400-403 DepthPeeler.rasterize_next_layer)',
    'texture.hip': 'nvdiffrast.texture / texture_construct_mip beyond the bilinear-clamp lookup of raster.hip (un-vendored; call sites render/texture.py:30,59-67 Texture2D.sample, render/light.py:64,76, render/util.py:190,201): mip pyramids, nearest / bilinear / trilinear filtering, wrap / clamp / zero / cube boundaries, gradients for texture levels, uv, uv_da, mip level bias',
    'material_grads.hip': 'smoothness buffers of shade(): render/render.py:72-74 (grad_weight), :88-91 (kd, kd_grad, ks_grad), :104-105 (nrm_grad) and their autograd',
    'aux_buffers.hip': 'forward-only buffers of a render layer: render/render.py:291-299 (z / z-gradient from the clip-space interpolation with derivatives), :197-199 (depth, inverse depth)',
    'act_ops.hip': 'MobileNetV2 perceptual trunk, conv-BN-ReLU6 blocks with the BatchNorm folded: geometry/hmsdf.py:137-159 (torchvision mobilenet_v2.features: nn.BatchNorm2d + nn.ReLU6 after every convolution but the linear projections)',
    'lpips_head.hip': 'LPIPS per-layer head: third_parties/lpips/lpips.py:112-134 (normalize_tensor, squared difference, lin layer, spatial_average) with third_parties/lpips/__init__.py:13-15',
    'image_ops.hip': 'render/mesh.py:418-446 (auto_normals), render/render.py:261-264 (face normals), render/renderutils/c_src/normal.cu:98,128 + torch_bindings.cpp (prepare_shading_normal_{fwd,bwd}), c_src/loss.cu:95,137 (image_loss_{fwd,bwd}), ssim_loss.py:33-63, geometry/hmsdf.py:162-170 (compute_sdf_reg_loss), render/render.py:375-382,430-449 (composite_buffer + loop), geometry/hmsdf.py:835-839,895-898,969-975,1064-1068 (per-pixel loss terms of tick_init / tick_split), kaolin.ops.mesh.sample_points (un-vendored; call sites geometry/hmsdf.py:714,750)',
    'bsdf.hip': 'render/renderutils/c_src/bsdf.cu + torch_bindings.cpp (lambert, frostbite, pbr_specular, pbr_bsdf, fresnel_shlick, ndf_ggx, lambda_ggx, masking_smith, each _{fwd,bwd}) with the semantics of the python twins render/renderutils/bsdf.py:57-151',
    'cubemap.hip': 'render/renderutils/c_src/cubemap.cu:110-169 (diffuse_cubemap_{fwd,bwd}), :246-350 (specular_cubemap_{fwd,bwd}) as driven by render/renderutils/ops.py:394-461; the backward as a gather',
    'bvh.hip': 'render/optixutils/c_src/optix_wrapper.cpp (optix_build_bvh: the OptiX acceleration structure) and the optixTrace of c_src/envsampling/kernel.cu:101-118 (any-hit shadow ray): a linear BVH built on the device and a stackless any-hit traversal -- the occlusion query is an entry point of its own',
    'bvhdist.hip': 'the pysdf queries of geometry/hmsdf.py:236-237 and script/process_body_cloth_head_msdfcut.py:683,744 answered from the tree of bvh.hip instead of mesh_ops.hip\'s loop over every triangle: node moments, the exact nearest triangle of a point, and the winding-signed distance with a first-order hierarchical winding number (Barill et al. 2018)',
    'envshade.hip': 'render/optixutils/c_src/envsampling/kernel.cu:463-542 (__raygen__rg: importance-sampled environment shading with shadow rays) + torch_bindings.cpp (env_shade_{fwd,bwd}), shaded with c_src/bsdf.h; driven by render/optixutils/ops.py:81-108',
    'denoise.hip': 'render/optixutils/c_src/denoising.cu:14-130 (bilateral_denoiser_{fwd,bwd}_kernel) as driven by render/optixutils/ops.py:110-122,145-147; a two-image form for the demodulated path of render/render.py:134-136 (one set of guides)',
    'envlight.hip': 'render/light.py:46-59 (EnvironmentLight.update_pdf: the pdf of the lat-long map and the row / column CDFs the light sampler of envshade.hip searches)',
    'mesh_ops.hip': 'seq-stage mesh terms: render/mesh.py:30-82 (compute_laplacian_uniform) + lap_loss.py:40-47 (body_laplacian_loss), render/mesh.py:18-28,266-279 (normal_consistency_loss), geometry/hmsdf.py:98-132 (collision_loss); start-up: geometry/hmsdf.py:236-237 (pysdf.SDF of the SMPL-X template on the grid vertices); stage hand-off: script/process_body_cloth_head_msdfcut.py:337-347 (deform_body_collision, one round) and the pysdf query of its Poisson-closed garment (:683,744) as a winding-signed distance to the open mesh',
    'meshtopo.hip': 'stage hand-off topology: script/connet_face_head.py:19-74 (UnionFind, find_connected_components), :97-112 (merge_and_repair_meshes: open3d remove_duplicated_vertices, un-vendored), script/process_body_cloth_head_msdfcut.py:92-102 (find_open_edges): lock-free union-find labelling, an exact-coordinate vertex weld and an edge-use count, each on an open-addressed table; error word bits 1 = face index out of range, 2 = iteration cap, 4 = table full',
    'meshrefine.hip': 'stage hand-off remeshing: the meshlabserver calls of script/process_body_cloth_head_msdfcut.py:621,625,661,715 with checkpoints/script/remesh.mlx (the refine step of isotropic remeshing) and :404-431 (process_subdivide) with midpoint_head.mlx (midpoint subdivision above an edge-length threshold): a conforming edge split on the edge table of meshtopo.hip, children in parent order; Jacobi relaxation of masked vertices for the caps of d3h/watertight.py (in place of the smoothness screened Poisson gives, wt.mlx)',
    'meshremesh.hip': 'stage hand-off remeshing, the rest of "Isotropic Explicit Remeshing" (checkpoints/script/remesh.mlx, the meshlabserver calls of script/process_body_cloth_head_msdfcut.py:621,625,661,715): edge collapse, edge flip and tangential smoothing on a sorted edge list and two CSR adjacencies, independent operations selected by a 64-bit atomic minimum per vertex (bit-reproducible); the refine step is meshrefine.hip, the reprojection Bvh.nearest of bvhdist.hip; counts word 2 is the error word (bit 1 = an index out of range)',
    'meshdecim.hip': 'level-of-detail export (no reference counterpart: train.py:198-246 writes the fitted mesh at one level of detail): quadric-error-metric edge collapse (Garland & Heckbert 1997) on the adjacency and the claim words of meshremesh.hip -- float64 quadrics gathered per vertex, cost and placement per edge, a cost window, selection by a 64-bit atomic minimum per vertex on (cost bucket, hashed rank), a trim to the target (bit-reproducible); face compaction is d3h_remesh_collapse_faces; counts word 2 is the error word (bit 1 = an index out of range)',
    'tetfill.hip': 'start-up: script/get_tet_smpl.py:9-27 (get_tet_mesh: tetgen behind pyvista, un-vendored) as called by geometry/hmsdf.py:239-249 -- not a constrained Delaunay mesh but a tet lattice clipped by the linear interpolant of a vertex field: inside vertices + the marching-tets cut vertices (same bits, same order), 0 / 1 / 3 / 3 / 1 children per parent, prisms split smallest id first; error word bit 1 = NaN in the field',
    'optim.hip': 'the optimiser step: train.py:747-748 (encoder gradient / 8), :759-768 (the two torch.optim.Adam steps of train.py:593-620), :788 + geometry/hmsdf.py:398-405 (clamp_deform)',
    'timing.hip': 'measurement only: per-launch HIP-event timing of selected kernels for bench.py (no reference counterpart; train.py:679,789-790 times whole iterations with time.time())',
    'gridenc.hip': 'tiny-cuda-nn Encoding beyond the one configuration of texmlp.hip (un-vendored; call site render/mlptexture.py:62-79,98): HashGrid / DenseGrid with any level count, 2-D / 3-D inputs, 1 / 2 / 4 / 8 features per entry, hashed levels, Linear / Smoothstep interpolation; gradients for the table and the positions',
    'fusedmlp.hip': 'tiny-cuda-nn Network (FullyFusedMLP / CutlassMLP; un-vendored) and the _MLP of render/mlptexture.py:18-41,100-103 for every shape texmlp.hip does not build: a bias-free MLP of 1..8 hidden layers of 16 / 32 / 64 / 128 neurons, seven activations, row mask, affine output map, forward and backward in one kernel each',
    'uvatlas.hip': 'textured-mesh export, train.py:198-246 (xatlas_uvmap: xatlas.parametrize, un-vendored, + render/render.py:456-472 render_uv + two util.dilate(.., 7)): a closed-form triangle-pair atlas and a position bake whose level-0 bilinear lookups never leave the triangle; render/texture.py:20-30 (texture2d_mip: 2 x 2 mean, the bilinear x2 upsample of 0.25 dout as its gradient rule)',
    'texmat.hip': 'the 2-D material lookups of shade(), render/render.py:277 (interpolate of v_tex by t_tex_idx) + render/texture.py:59-67 (Texture2D.sample of kd, ks, normal) at level 0: texel coordinate and up to three bilinear lookups per pixel in one pass, map gradients by fp32 atomics',
    'texmlp.hip': 'render/mlptexture.py:91-107 (MLPTexture3D.sample): tiny-cuda-nn HashGrid encoding (:62-79, un-vendored) + _MLP (:18-41) + sigmoid range map',
}
ORDER = ['sdf_mlp.hip', 'sdf_mlp_x3.hip', 'sdf_mlp_bwd.hip', 'marching_tets.hip', 'lbs.hip', 'smplx_pose.hip', 'raster.hip', 'texture.hip', 'aux_buffers.hip', 'material_grads.hip', 'image_ops.hip', 'bsdf.hip', 'cubemap.hip', 'bvh.hip', 'bvhdist.hip', 'envshade.hip', 'envlight.hip', 'denoise.hip', 'lpips_head.hip', 'act_ops.hip', 'mesh_ops.hip', 'meshtopo.hip', 'meshrefine.hip', 'meshremesh.hip', 'meshdecim.hip', 'tetfill.hip', 'texmlp.hip', 'gridenc.hip', 'fusedmlp.hip', 'uvatlas.hip', 'texmat.hip', 'optim.hip', 'timing.hip']
head = '''/* d3h.h -- C ABI of libd3h_hip.so: the MI355X (gfx950) hot path of D3-Human's render-and-fit loop.
 * GENERATED by tools/gen_header.py from the extern "C" definitions in d3human-code_amd/csrc/ -- do not edit by hand.
 *
 * Conventions (mirroring the reference's native plugin, render/renderutils/c_src/torch_bindings.cpp:25-41):
 *  - every pointer is a DEVICE pointer into memory owned by the caller (PyTorch-ROCm allocations) unless a comment says HOST;
 *    tensors are contiguous row-major; float = fp32, indices int32 unless stated;
 *  - `stream` is a hipStream_t; kernels are enqueued on it and the call returns without synchronising;
 *  - return 0 on success, <0 for an argument error, >0 = hipError_t of a failed launch (the Python wrappers raise RuntimeError,
 *    as TORCH_CHECK does in the reference);
 *  - data-dependent output sizes are returned through small device counters the caller reads back (marching tets);
 *  - "accumulated" outputs are added to (caller zero-fills or passes .grad buffers), "overwritten" outputs are fully written.
 */
#ifndef D3H_H
#define D3H_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
'''
ver = re.search(r'#define D3H_ABI_VERSION (\d+)', open(os.path.join(ROOT, 'd3human-code_amd', 'csrc', 'd3h_common.h')).read()).group(1)
head = head + f'''
/* ABI version: bumped whenever an entry point changes its signature or disappears; compare with d3h_abi_version() of the loaded library
 * (history: INTEGRATION.md, "ABI history") */
#define D3H_ABI_VERSION {ver}
'''
out = [head]
sigs = []                      # every declaration, in header order: the rows of d3h/_abi.py
for fn in ORDER:
    s = open(os.path.join(ROOT, 'd3human-code_amd', 'csrc', fn)).read()
    out.append(f'\n/* ==== {fn}: replaces {GROUPS[fn]} ==== */\n')
    for m in re.finditer(r'((?:[ \t]*//[^\n]*\n)*)extern "C" ([^{;]+?)\s*\{', s):
        comment = ''.join('/* ' + l.strip()[2:].strip() + ' */\n' for l in m.group(1).splitlines() if l.strip() and not l.strip().startswith('// ---'))
        sig = ' '.join(m.group(2).split())
        out.append(comment + sig + ';\n')
        sigs.append(sig)
# compile-time variants: the same sources built a second time under other entry-point names (see csrc/deform_mlp*.hip)
VARIANTS = [('deform_mlp.hip', 'sdf_mlp.hip', 'offset network MLP_deform: geometry/mlp.py:77-118 (seq stage, geometry/hmsdf.py:658-665); sdf_mlp.hip compiled '
             'with a 51-wide encoding and a 3-output head, the 136-float pose code folded into the first bias by the caller'),
            ('deform_mlp_bwd.hip', 'sdf_mlp_bwd.hip', 'backward of the offset network (sdf_mlp_bwd.hip, same configuration): gout [n][3], dw0 [256][51], '
             'dw4 [256][307], dw7 [3][256], db7 [3]')]
for wrapper, base, what in VARIANTS:
    w = open(os.path.join(ROOT, 'd3human-code_amd', 'csrc', wrapper)).read()
    ren = dict(re.findall(r'#define (d3h_sdf_mlp\w+) (d3h_deform_mlp\w+)', w))
    s = open(os.path.join(ROOT, 'd3human-code_amd', 'csrc', base)).read()
    out.append(f'\n/* ==== {wrapper}: {what} ==== */\n')
    for m in re.finditer(r'extern "C" ([^{;]+?)\s*\{', s):
        sig = ' '.join(m.group(1).split())
        name = re.search(r'\b(d3h_\w+)\s*\(', sig).group(1)
        if name in ren:
            out.append(sig.replace(name, ren[name]) + ';\n')
            sigs.append(sig.replace(name, ren[name]))
out.append('\n#ifdef __cplusplus\n}\n#endif\n#endif\n')
open(os.path.join(ROOT, 'include', 'd3h.h'), 'w').write(''.join(out))
print('wrote include/d3h.h')

# ---- d3h/_abi.py: {name: (return type, ((C type, parameter name), ...))}.  A name declared twice (timing.hip: the emulation's stubs
# carry no parameter names) is one row, the declaration with names
abi = {}
for sig in sigs:
    ret, name, params = re.fullmatch(r'(.+?)\s*\b(d3h_\w+)\s*\((.*)\)', sig).groups()
    row = []
    for p in ([] if params.strip() in ('', 'void') else params.split(',')):
        m = re.fullmatch(r'\s*(.*?[\s*])(\w+)\s*', p)
        ctype, pname = (m.group(1), m.group(2)) if m and m.group(2) not in ('int', 'long', 'int64_t', 'float', 'double', 'unsigned') else (p, '')
        row.append((' '.join(ctype.split()), pname))
    if name not in abi or all(n for _, n in row):
        abi[name] = (ret, tuple(row))
lines = ['"""Signatures of the C ABI (include/d3h.h) as data: {entry point: (return type, ((C type, parameter name), ...))}.\n'
         'GENERATED by tools/gen_header.py from the extern "C" definitions in d3human-code_amd/csrc/ -- do not edit by hand."""\n', 'ABI = {\n']
for name, (ret, row) in abi.items():
    lines.append(f'    {name!r}: ({ret!r}, ({"".join(repr(r) + ", " for r in row)})),\n')
lines.append('}\n')
open(os.path.join(ROOT, 'd3human-code_amd', 'd3h', '_abi.py'), 'w').write(''.join(lines))
print('wrote d3human-code_amd/d3h/_abi.py')
