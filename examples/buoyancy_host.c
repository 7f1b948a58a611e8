/* buoyancy_host.c -- a box floating on the generator's maps, from plain C99: the hull and the per-point state stay on the device, every
 * physics step uploads one 96-byte pose, enqueues ow_buoyancy_async with the warm start, and reads back one 64-byte result, which a
 * semi-implicit Euler integrator turns into the next pose.
 *   gcc -O2 -std=c99 -Iinclude examples/buoyancy_host.c -o buoyancy_host -Lgodotoceanwaves_amd -locean_waves -L/opt/rocm/lib -lamdhip64 \
 *       -Wl,-rpath,$PWD/godotoceanwaves_amd -Wl,-rpath,/opt/rocm/lib -lm && ./buoyancy_host [calm|demo [steps]]
 * calm: no displacement (map_scales.z = 0), the water is the plane y = 0; a box of half the water's density must settle at half its
 * height.  demo: the three cascades of the reference's main.tscn, advanced every step; the box must stay afloat and finite.
 * Prints key=value pairs: the final draft and the one Archimedes predicts, the range of heights the box's origin visited, the mean
 * submerged share, whether everything stayed finite and the box afloat, and the mean Newton evaluations per hull point of the last step
 * (the warm start's effect). */
#include "scene.h"

#define NX 4
#define NY 4
#define NZ 4
#define NPOINTS (NX * NY * NZ)

static void mat_mul(const double a[9], const double b[9], double out[9]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

/* R <- exp([w dt]x) R (Rodrigues), then Gram-Schmidt on the rows so that rounding does not shear the box */
static void rotate(double R[9], const double w[3], double dt) {
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) * dt;
    if (th > 0.0) {
        const double k[3] = {w[0] * dt / th, w[1] * dt / th, w[2] * dt / th};
        const double K[9] = {0, -k[2], k[1], k[2], 0, -k[0], -k[1], k[0], 0};
        double K2[9], E[9], out[9];
        mat_mul(K, K, K2);
        for (int i = 0; i < 9; ++i) E[i] = (i % 4 == 0 ? 1.0 : 0.0) + sin(th) * K[i] + (1.0 - cos(th)) * K2[i];
        mat_mul(E, R, out);
        memcpy(R, out, sizeof out);
    }
    for (int i = 0; i < 3; ++i) {
        double *r = R + 3 * i;
        for (int j = 0; j < i; ++j) {
            const double *q = R + 3 * j, d = r[0] * q[0] + r[1] * q[1] + r[2] * q[2];
            for (int c = 0; c < 3; ++c) r[c] -= d * q[c];
        }
        const double n = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        for (int c = 0; c < 3; ++c) r[c] /= n;
    }
}

int main(int argc, char **argv) {
    const int demo = argc > 1 && strcmp(argv[1], "demo") == 0, steps = argc > 2 ? atoi(argv[2]) : 300;
    const int n = 256, cascades = SCENE_CASCADES;
    const double dt = 1.0 / 60.0, g = 9.81, rho = 1025.0;
    const double size[3] = {2.0, 1.0, 2.0}, volume = size[0] * size[1] * size[2], mass = 0.5 * rho * volume;
    const double inertia[3] = {mass / 12.0 * (size[1] * size[1] + size[2] * size[2]), mass / 12.0 * (size[0] * size[0] + size[2] * size[2]),
                               mass / 12.0 * (size[0] * size[0] + size[1] * size[1])};
    int status = 1;
    void *hull_dev = NULL, *body_dev = NULL, *result_dev = NULL, *points_dev = NULL;

    ow_config cfg;
    scene_config(&cfg, n);
    ow_context *ctx = NULL;
    if (ow_create(&cfg, &ctx) != OW_OK) { fprintf(stderr, "ow_create: %s\n", ow_last_error()); return 1; }

    ow_cascade_params par[SCENE_CASCADES];
    float map_scales[SCENE_CASCADES][4];
    scene_cascades(par, map_scales);
    if (!demo)
        for (int i = 0; i < cascades; ++i) map_scales[i][2] = 0.0f;   /* calm: no displacement at all */

    /* the hull: the box voxelised into NX x NY x NZ cells, one point per cell with the cell's volume and half its height */
    ow_hull_point hull[NPOINTS];
    memset(hull, 0, sizeof hull);
    for (int i = 0, k = 0; i < NX; ++i)
        for (int j = 0; j < NY; ++j)
            for (int l = 0; l < NZ; ++l, ++k) {
                hull[k].local[0] = (float)((i + 0.5) * size[0] / NX - size[0] / 2);
                hull[k].local[1] = (float)((j + 0.5) * size[1] / NY - size[1] / 2);
                hull[k].local[2] = (float)((l + 0.5) * size[2] / NZ - size[2] / 2);
                hull[k].volume = (float)(volume / NPOINTS);
                hull[k].half_height = (float)(size[1] / NY / 2);
                hull[k].body = 0;
            }
    if (hipMalloc(&hull_dev, sizeof hull) || hipMalloc(&body_dev, sizeof(ow_buoyancy_body)) || hipMalloc(&result_dev, sizeof(ow_buoyancy_result)) ||
        hipMalloc(&points_dev, NPOINTS * sizeof(ow_buoyancy_point)) || hipMemcpy(hull_dev, hull, sizeof hull, HIP_HOST_TO_DEVICE)) {
        fprintf(stderr, "hipMalloc / hipMemcpy failed\n");
        goto out;
    }
    {   /* zeros: the first step starts cold */
        static ow_buoyancy_point zeros[NPOINTS];
        if (hipMemcpy(points_dev, zeros, sizeof zeros, HIP_HOST_TO_DEVICE)) { fprintf(stderr, "hipMemcpy failed\n"); goto out; }
    }
    ow_buoyancy_options opts;
    memset(&opts, 0, sizeof opts);
    opts.flags = OW_BUOYANCY_WARM_START;   /* density 1025, gravity 9.81, water level 0: the defaults */

    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, o[3] = {5.0, 0.3, -3.0}, v[3] = {0, 0, 0}, w[3] = {0, 0, 0};
    double y_min = 1e30, y_max = -1e30, wet_share = 0.0, evals = 0.0;
    int finite = 1;
    ow_buoyancy_result res;
    memset(&res, 0, sizeof res);
    for (int step = 0; step < steps; ++step) {
        if (demo && ow_update_all(ctx, dt, par, cascades) != OW_OK) goto fail;
        ow_buoyancy_body body;
        memset(&body, 0, sizeof body);
        for (int i = 0; i < 9; ++i) body.transform[i] = (float)R[i];
        for (int i = 0; i < 3; ++i) {
            body.transform[9 + i] = (float)o[i];
            body.linear_velocity[i] = (float)v[i];
            body.angular_velocity[i] = (float)w[i];
        }
        body.point_offset = 0; body.point_count = NPOINTS;
        body.linear_drag = 3.0f; body.quadratic_drag = 0.5f;
        if (hipMemcpy(body_dev, &body, sizeof body, HIP_HOST_TO_DEVICE)) { fprintf(stderr, "hipMemcpy failed\n"); goto out; }
        if (ow_buoyancy_async(ctx, (const ow_buoyancy_body *)body_dev, 1, (const ow_hull_point *)hull_dev, NPOINTS, &map_scales[0][0], cascades, &opts,
                              (ow_buoyancy_result *)result_dev, (ow_buoyancy_point *)points_dev) != OW_OK)
            goto fail;
        if (ow_sync(ctx) != OW_OK) goto fail;
        if (hipMemcpy(&res, result_dev, sizeof res, HIP_DEVICE_TO_HOST)) { fprintf(stderr, "hipMemcpy failed\n"); goto out; }
        if (step == steps - 1 || step % 50 == 0) {   /* what the warm start costs: the per-point records say */
            static ow_buoyancy_point pts[NPOINTS];
            double e = 0.0;
            if (hipMemcpy(pts, points_dev, sizeof pts, HIP_DEVICE_TO_HOST)) { fprintf(stderr, "hipMemcpy failed\n"); goto out; }
            for (int i = 0; i < NPOINTS; ++i) e += pts[i].evaluations;
            if (step == steps - 1) evals = e / NPOINTS;
        }
        /* semi-implicit Euler: velocities from the forces of this pose, then the pose from the new velocities */
        double Iinv_w[9], tmp[9], Rt[9], Dinv[9] = {1 / inertia[0], 0, 0, 0, 1 / inertia[1], 0, 0, 0, 1 / inertia[2]};
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Rt[3 * i + j] = R[3 * j + i];
        mat_mul(R, Dinv, tmp);
        mat_mul(tmp, Rt, Iinv_w);   /* world-space inverse inertia R I^-1 R^T */
        for (int i = 0; i < 3; ++i) v[i] += dt * res.force[i] / mass;
        v[1] -= dt * g;
        for (int i = 0; i < 3; ++i) w[i] += dt * (Iinv_w[3 * i] * res.torque[0] + Iinv_w[3 * i + 1] * res.torque[1] + Iinv_w[3 * i + 2] * res.torque[2]);
        for (int i = 0; i < 3; ++i) o[i] += dt * v[i];
        rotate(R, w, dt);
        for (int i = 0; i < 3; ++i) finite &= isfinite(o[i]) && isfinite(v[i]) && isfinite(w[i]) && isfinite(res.force[i]) && isfinite(res.torque[i]);
        if (o[1] < y_min) y_min = o[1];
        if (o[1] > y_max) y_max = o[1];
        wet_share += res.submerged_volume / volume / steps;
    }
    {
        /* upright box: the bottom face is at o.y - R[4] * size.y / 2 */
        const double draft = -(o[1] - R[4] * size[1] / 2), expected = 0.5 * size[1];
        /* afloat: riding the waves (the origin stays within a few metres of the mean level, which troughs and crests leave by
         * a metre or two) and about half in the water on average */
        const int afloat = finite && y_min > -5.0 && y_max < 5.0 && wet_share > 0.2 && wet_share < 0.8;
        printf("steps=%d draft=%.5f expected_draft=%.5f y_min=%.4f y_max=%.4f submerged_share=%.4f invalid_points=%d evaluations_per_point=%.3f "
               "finite=%d afloat=%d\n", steps, draft, expected, y_min, y_max, wet_share, res.invalid_points, evals, finite, afloat);
    }
    status = 0;
    goto out;
fail:
    fprintf(stderr, "ocean_waves: %s\n", ow_last_error());
out:
    (void)hipFree(hull_dev); (void)hipFree(body_dev); (void)hipFree(result_dev); (void)hipFree(points_dev);
    ow_destroy(ctx);
    return status;
}
