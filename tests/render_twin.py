"""FP64 twin of the water shader's shading: assets/shaders/spatial/water.gdshader fragment() lines 73-93 past the texture reads and
light() lines 96-127, restated in NumPy float64 from the shader text (GLSL's mix, smoothstep, pow, normalize as the GLSL specification
defines them), plus the pixel-ray formula and the composite of include/ocean_waves.h ow_render_view.  It does not start from
csrc/ow_shading.h and carries none of its guards: where GLSL divides by zero this divides by zero (tests feed it the record's own inputs
and compare where the twin is finite, and say so)."""
import numpy as np

REFLECTANCE = 0.02   # :9


def mix(a, b, t):
    return a * (1.0 - t) + b * t


def smoothstep(e0, e1, x):
    t = np.clip((x - e0) / (e1 - e0), 0.0, 1.0)
    return t * t * (3.0 - 2.0 * t)


def normalize(v):
    return v / np.sqrt((v * v).sum(axis=-1))[..., None]


def dot(a, b):
    return (a * b).sum(axis=-1)


def pixel_directions(basis, fov_y_degrees, width, height):
    """unit directions [H][W][3] of the rays through the pixel centres: B * ((2 (i + 0.5) / W - 1) * aspect * tan(fov / 2),
    (1 - 2 (j + 0.5) / H) * tan(fov / 2), -1), normalised"""
    B = np.asarray(basis, np.float64).reshape(3, 3)
    th = np.tan(np.radians(np.float64(fov_y_degrees)) / 2.0)
    i = np.arange(width, dtype=np.float64)[None, :]
    j = np.arange(height, dtype=np.float64)[:, None]
    x = (2.0 * (i + 0.5) / width - 1.0) * (width / height) * th + 0.0 * j
    y = (1.0 - 2.0 * (j + 0.5) / height) * th + 0.0 * i
    local = np.stack([x, y, -np.ones_like(x)], axis=-1)
    return normalize(local @ B.T)


def smith_masking_shadowing(cos_theta, alpha):   # :96-100
    with np.errstate(divide="ignore", invalid="ignore"):
        a = cos_theta / (alpha * np.sqrt(1.0 - cos_theta * cos_theta))
        a_sq = a * a
        return np.where(a < 1.6, (1.0 - 1.259 * a + 0.396 * a_sq) / (3.535 * a + 2.181 * a_sq), 0.0)


def ggx_distribution(cos_theta, alpha):          # :103-107
    a_sq = alpha * alpha
    d = 1.0 + (a_sq - 1.0) * cos_theta * cos_theta
    with np.errstate(divide="ignore", invalid="ignore"):
        return a_sq / (np.pi * d * d)


def shade(gradient_fragment, foam_fragment, wave_height, position, cam_position, cam_basis, uniforms):
    """fragment() from :74 on and light() for arrays of surface points.  gradient_fragment [..., 2], foam_fragment, wave_height [...]:
    the sums of :76-84 and :38 at the point's UV; position [..., 3] world; cam_basis: Transform3D basis rows.  uniforms: water_color,
    foam_color, roughness, normal_strength, light_direction (towards the light, any length), light_color, ambient_color.  NORMAL, VIEW
    and LIGHT are kept in world space: the shader's view-space rotation changes no dot product."""
    f64 = lambda v: np.asarray(v, np.float64)   # noqa: E731
    g = f64(gradient_fragment)
    foam, wave_height, pos = f64(foam_fragment), f64(wave_height), f64(position)
    B = f64(cam_basis).reshape(3, 3)
    water_color, foam_color = f64(uniforms["water_color"]), f64(uniforms["foam_color"])
    roughness, normal_strength = float(uniforms["roughness"]), float(uniforms["normal_strength"])
    LIGHT = normalize(f64(uniforms["light_direction"]))
    LIGHT_COLOR = f64(uniforms["light_color"])
    rel = pos - f64(cam_position)
    vertex_view = rel @ B                                   # VIEW_MATRIX * world: the components along the basis columns
    VIEW = normalize(-rel)
    dist = np.sqrt(vertex_view[..., 0] ** 2 + vertex_view[..., 2] ** 2)                       # :74
    foam_factor = smoothstep(0.0, 1.0, foam * 0.75) * np.exp(-dist * 0.0075)                  # :86
    ALBEDO = mix(water_color, foam_color, foam_factor[..., None])                              # :87
    g = g * mix(0.015, normal_strength, np.exp(-dist * 0.0175))[..., None]                     # :89
    NORMAL = normalize(np.stack([-g[..., 0], np.ones_like(dist), -g[..., 1]], axis=-1))        # :90
    with np.errstate(invalid="ignore"):
        fresnel = mix(np.power(1.0 - dot(VIEW, NORMAL), 5.0 * np.exp(-2.69 * roughness)) / (1.0 + 22.7 * roughness ** 1.5), 1.0, REFLECTANCE)   # :92
    ROUGHNESS = (1.0 - fresnel) * foam_factor + 0.4                                            # :93
    with np.errstate(divide="ignore", invalid="ignore"):
        halfway = normalize(LIGHT + VIEW)                                                      # :110
        dot_nl = np.maximum(dot(NORMAL, LIGHT), 2e-5)                                          # :111
        dot_nv = np.maximum(dot(NORMAL, VIEW), 2e-5)                                           # :112
        light_mask = smith_masking_shadowing(roughness, dot_nv)                                # :115, the arguments as written
        view_mask = smith_masking_shadowing(roughness, dot_nl)                                 # :116
        microfacet_distribution = ggx_distribution(dot(NORMAL, halfway), roughness)            # :117
        geometric_attenuation = 1.0 / (1.0 + light_mask + view_mask)                           # :118
        SPECULAR = fresnel * microfacet_distribution * geometric_attenuation / (4.0 * dot_nv + 0.1)   # :119, ATTENUATION 1
        sss_modifier = np.array([0.9, 1.15, 0.85])                                             # :122
        sss_height = (1.0 * np.maximum(0.0, wave_height + 2.5) * np.power(np.maximum(dot(LIGHT, -VIEW), 0.0), 4.0)
                      * np.power(0.5 - 0.5 * dot(LIGHT, NORMAL), 3.0))                          # :123
        sss_near = 0.5 * np.power(dot_nv, 2.0)                                                 # :124
        lambertian = 0.5 * dot_nl                                                              # :125
        lit = (sss_height + sss_near)[..., None] * sss_modifier / (1.0 + light_mask)[..., None] + lambertian[..., None]
        DIFFUSE = mix(lit, foam_color, foam_factor[..., None]) * (1.0 - fresnel)[..., None] * LIGHT_COLOR   # :126
    color = ALBEDO * (DIFFUSE + f64(uniforms["ambient_color"])) + SPECULAR[..., None]          # ow_render_view's composite
    return {"dist": dist, "foam_factor": foam_factor, "albedo": ALBEDO, "normal": NORMAL, "fresnel": fresnel, "roughness": ROUGHNESS,
            "diffuse": DIFFUSE, "specular": SPECULAR, "color": color}


def rgba8(color):
    c = np.clip(np.asarray(color, np.float64), 0.0, 1.0)
    out = np.full(c.shape[:-1] + (4,), 255, np.uint8)
    out[..., :3] = np.floor(c * 255.0 + 0.5).astype(np.uint8)
    return out
