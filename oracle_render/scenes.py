"""Obstacle sets for the tests of the rendered map -- TEST INFRASTRUCTURE: the small grid, named shapes where the kernels can go wrong,
and seeded random polygons of every kind (convex, concave, self-crossing, with repeated vertices, with collinear runs, partly and
wholly outside).  Only tests/ and scripts/ import this."""
import numpy as np

SX, SY, RES, ORG = 70, 40, 0.1, (-1.3, 0.7)      # 70 x 40 cells: a bit map, and 70 % 32 != 0


def world(cells, res=RES, org=ORG):
    """world coordinates of cell coordinates [n][2] (cell centres, so that they snap back to themselves)"""
    c = np.asarray(cells, dtype=np.float64).reshape(-1, 2)
    return np.stack([org[0] + c[:, 0] * res, org[1] + c[:, 1] * res], axis=1)


def pack(polys):
    """a list of [n_k][2] arrays -> (poly_xy [sum n_k][2], poly_off [len + 1] int32)"""
    off = np.concatenate([[0], np.cumsum([len(p) for p in polys])]).astype(np.int32)
    xy = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in polys]) if len(polys) else np.zeros((0, 2))
    return xy, off


def named():
    """the shapes of the small grid, in cells: name -> a list of polygons (world coordinates)"""
    ring = [(35 + 14 * np.cos(a), 20 + 12 * np.sin(a)) for a in np.linspace(0.0, 2.0 * np.pi, 64, endpoint=False)]
    s = {
        "triangle": [[(10, 5), (40, 9), (22, 33)]],
        "L": [[(8, 6), (30, 6), (30, 14), (16, 14), (16, 34), (8, 34)]],
        "bow-tie": [[(10, 8), (50, 30), (50, 8), (10, 30)]],
        "square on integers": [[(20, 10), (45, 10), (45, 30), (20, 30)]],
        "64 vertices": [ring],
        "left border": [[(-8, 10), (12, 14), (5, 30)]],
        "right border": [[(60, 5), (80, 12), (64, 28)]],
        "lower border": [[(20, -9), (44, -3), (30, 12)]],
        "upper border": [[(15, 30), (40, 36), (28, 52)]],
        "corner at the origin": [[(-10, -6), (14, -3), (6, 9), (-4, 12)]],
        "far corner": [[(60, 30), (85, 35), (75, 50), (62, 44)]],
        "wholly outside": [[(100, 10), (140, 12), (120, 30)], [(10, -50), (30, -44), (20, -20)], [(-3000, 5), (-2000, 8), (-2500, 30)]],
        "two vertices": [[(5, 5), (48, 31)]],
        "one vertex": [[(33, 17)], [(200, 3)]],
        "no vertices among others": [[(10, 5), (20, 5), (15, 15)], np.zeros((0, 2)), [(40, 20), (60, 22), (50, 35)]],
        "a span over the whole row": [[(-20, 5), (100, 5), (100, 25), (-20, 25)]],
        "closed by a repeated vertex": [[(4, 4), (8, 4), (8, 8), (4, 8), (4, 4)]],
    }
    return {k: [world(p) for p in v] for k, v in s.items()}


def random_polygon(rng):
    """one polygon in world coordinates on the small grid, and its kind"""
    kind = ("convex", "concave", "self-crossing", "repeated", "collinear")[int(rng.integers(5))]
    where = ("inside", "partly", "outside")[int(rng.choice(3, p=[0.5, 0.35, 0.15]))]
    cx, cy = {"inside": (rng.uniform(15, 55), rng.uniform(10, 30)),
              "partly": (rng.choice([-2.0, 72.0, rng.uniform(0, 70)]), rng.choice([-2.0, 41.0, rng.uniform(0, 40)])),
              "outside": (rng.choice([-40.0, 120.0]), rng.choice([-30.0, 80.0]))}[where]
    n = int(rng.integers(3, 13))
    ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, n))
    rad = rng.uniform(4.0, 14.0)
    if kind == "concave":
        r = rad * np.where(np.arange(n) % 2 == 0, 1.0, rng.uniform(0.25, 0.6))
    else:
        r = np.full(n, rad)
    pts = np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], axis=1)
    if kind == "self-crossing":
        pts = pts[rng.permutation(n)]
    pts = np.rint(pts + rng.uniform(-0.5, 0.5, pts.shape) * (rng.random() < 0.5))       # half of them on cell centres
    if kind == "repeated":
        pts = np.repeat(pts, rng.integers(1, 4, n), axis=0)
    if kind == "collinear":                                                             # the midpoints of the edges, and the ends twice over
        mid = 0.5 * (pts + np.roll(pts, -1, axis=0))
        pts = np.stack([pts, mid], axis=1).reshape(-1, 2)
    pts = pts + rng.uniform(-0.5, 0.5, pts.shape) * (rng.random() < 0.3)                # some off the centres, halves included
    return world(pts[:64]), kind + " " + where


def random_polygons(seed, n=200):
    rng = np.random.default_rng(seed)
    return [random_polygon(rng) for _ in range(n)]
