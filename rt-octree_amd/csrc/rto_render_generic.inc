// rto_render_generic.inc -- body of the generic kernel, included by frame_kernels.hip into render_generic (a camera's pixels)
// render_rays_generic (RTO_GENERIC_RAYS defined to 1 around the include: the rays of rto_launch_rays) and render_generic_layers
// (RTO_GENERIC_LAYERS defined to 1: a camera's pixels over the layers of rto_ctx_set_layers).  In scope: the kernel
// parameters and SPP.  (The ray source is switched by the preprocessor: render_generic's text and code are unchanged.)
// RTO_DEPTH defined to 1 as well (render_rays_generic_depth, render_generic_layers_depth): the distance of the ray's hits, d = t *
// delta_scale at the top of the iteration that collides, goes to `dout` (DepthOut; include/rto.h "depth outputs").  This loop is
// the reference's own arithmetic: its values define the two outputs.
#if RTO_GENERIC_RAYS
    const uint32_t ray = ray_index(rays, blockIdx.x, threadIdx.x);
    if (ray >= rays.n) return;
    float out[4] = {0.f, 0.f, 0.f, 0.f};
#if RTO_DEPTH
    float dsum = 0.f, tnear = __builtin_inff();
#endif
    float dir[3], vdir[3], cen[3], invdir[3], tmax_bg, bg[3];
    const bool live = ray_from_batch(rays, ray, tree, opt.background_brightness, dir, vdir, cen, tmax_bg, bg);  // (false: degenerate)

    if (tree.N > 0 && live) {  // enable_draw volrend.cu:98
        Pcg32 rng = rng_base;
        pcg_advance(rng, (int64_t)ray * SPP);  // volrend.cu:157
        float delta_scale, tmin, tmax;
        if (ray_enter(tree, opt, dir, cen, tmax_bg, invdir, delta_scale, tmin, tmax)) {
#elif RTO_GENERIC_LAYERS
    const int64_t SIZE = (int64_t)cam.width * cam.height;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= SIZE) return;
    const int x = idx % cam.width, y = idx / cam.width;
    float out[4] = {0.f, 0.f, 0.f, 0.f};
#if RTO_DEPTH
    float dsum = 0.f, tnear = __builtin_inff();
#endif
    float dir[3], vdir[3], cen[3], invdir[3], bg[3];
    layer_backdrop(layers, (uint32_t)idx, opt.background_brightness, bg);
    ray_setup(x, y, cam, tree, dir, vdir, cen);
    const float tmax_bg = layers.depth ? layers.depth[idx] : 1e9f;
    const bool live = ray_is_live(tmax_bg, dir, cen);  // (false: not traced, as a degenerate ray of rto_launch_rays)

    if (tree.N > 0 && live) {  // enable_draw volrend.cu:98
        Pcg32 rng = rng_base;
        pcg_advance(rng, (int64_t)(idx * SPP));  // volrend.cu:157
        float delta_scale, tmin, tmax;
        if (ray_enter(tree, opt, dir, cen, tmax_bg, invdir, delta_scale, tmin, tmax)) {
#else
    const int64_t SIZE = (int64_t)cam.width * cam.height;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= SIZE) return;
    const int x = idx % cam.width, y = idx / cam.width;
    float out[4] = {0.f, 0.f, 0.f, 0.f};

    if (tree.N > 0) {  // enable_draw volrend.cu:98
        float dir[3], vdir[3], cen[3], invdir[3];
        ray_setup(x, y, cam, tree, dir, vdir, cen);
        Pcg32 rng = rng_base;
        pcg_advance(rng, (int64_t)(idx * SPP));  // volrend.cu:157
        float delta_scale, tmin, tmax;
        if (ray_enter(tree, opt, dir, cen, 1e9f, invdir, delta_scale, tmin, tmax)) {
#endif
            // sample_dst rt_core.cuh:67-193
            float dst[SPP + 1];
            for (int n = 1; n <= SPP; ++n) {
                const float tv = -det_log_one_minus(pcg_next_float(rng));
                if (n == 1) {
                    dst[0] = tv;
                } else if (tv <= dst[0]) {
                    for (int i = n - 1; i > 0; i--) dst[i] = dst[i - 1];
                    dst[0] = tv;
                } else {
                    int i = n - 1;
                    while (dst[i - 1] > tv) {
                        dst[i] = dst[i - 1];
                        i--;
                    }
                    dst[i] = tv;
                }
            }
            dst[SPP] = 3.402823466e+38f;

            int64_t tree_vals[SPP];
            float cnts[SPP];
            for (int i = 0; i < SPP; ++i) cnts[i] = 0.f;
            uint32_t spp = 0, sh_nums = 0;
            float src = 0;
            float t = tmin;
            while (t < tmax) {  // rt_core.cuh:241-270
                float pos[3] = {cen[0] + t * dir[0], cen[1] + t * dir[1], cen[2] + t * dir[2]};
                float cube_sz;
                const int64_t leaf = query_from_root(tree, pos, cube_sz);
                const float t_subcube = dda_unit(pos, invdir) / cube_sz;
                const float delta_t = t_subcube + opt.step_size;
                const float sigma = half_bits_to_float(tree.data[leaf * tree.data_dim + tree.data_dim - 1]);
                if (sigma > opt.sigma_thresh) {
                    const float delta = delta_t * delta_scale * sigma;
                    if (src + delta >= dst[spp]) {
                        float& cnt = cnts[sh_nums];
                        tree_vals[sh_nums] = leaf;
                        ++sh_nums;
                        do {
                            ++cnt;
                            ++spp;
                        } while (src + delta >= dst[spp]);
#if RTO_DEPTH
                        {
                            const float d = t * delta_scale;
                            dsum += cnt * d;
                            tnear = sh_nums == 1u ? d : tnear;  // (sh_nums counts this hit already)
                        }
#endif
                        if (spp == SPP) break;
                    }
                    src += delta;
                }
                t += delta_t;
            }
#if RTO_DEPTH
            dsum *= 1.0f / SPP;
#endif
#if RTO_DEPTH && RTO_GENERIC_RAYS
            if (sh_nums != 0 && rays.out) {  // (uniform: a call that asks for no colour shades nothing)
#else
            if (sh_nums != 0) {
#endif
                float basis_fn[RTO_BASIS_MAX_DEV];
                ray_basis_any(tree, opt, vdir, basis_fn);
                for (uint32_t i = 0; i < sh_nums; i++)
                    shade_leaf(tree, tree.data + tree_vals[i] * tree.data_dim, basis_fn, cnts[i], out);
                constexpr float INV_SPP = 1.0f / SPP;
                out[0] *= INV_SPP;
                out[1] *= INV_SPP;
                out[2] *= INV_SPP;
                out[3] *= INV_SPP;
            }
        }
    }
#if RTO_GENERIC_RAYS && RTO_DEPTH
    if (rays.out) write_ray(rays, ray, bg, out);
    write_depth(dout, ray, dsum, tnear);
#elif RTO_GENERIC_RAYS
    write_ray(rays, ray, bg, out);
#elif RTO_GENERIC_LAYERS
    write_pixel_over(fo, SIZE, idx, bg, out);
#if RTO_DEPTH
    write_depth(dout, (uint32_t)idx, dsum, tnear);
#endif
#else
    write_pixel(fo, SIZE, idx, opt.background_brightness, out);
#endif
