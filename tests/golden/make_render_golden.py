#!/usr/bin/env python3
"""Record the reference's picture (this container only): the render_* fixtures and render_atlas.json.

The real reference is imported read-only with the shims of ./shims, as make_golden.py does, and its
OpencvRenderer.render is run on the world after every recorded call with cv2.imshow replaced by a capture.  Nothing of
the reference is copied: only pixels it drew are written.

  render_atlas.json   the five 11 x 11 masks and the six colours, read off the reference's own draws of one thing each
                      on a black 30 x 30 image
  render_*.json.gz    fixtures in make_golden.py's format (golden_driver.run_config; the calls' records are exactly that
                      driver's, so every replay of the fixtures reads them), every run with a "render" list besides,
                      one record per call: "hash" (the first 64 bits of the sha256 of the frame cropped to the map area), "bodies"
                      ([x, y, palette index] of every DeadBody of World.decoration) and, for three calls of the first
                      seed, "frame": the cropped frame packed as one palette index per pixel (255: black), zlib + base64

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_render_golden.py
"""
import base64
import gzip
import hashlib
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402  (puts the shims and the reference on the path)
import golden_driver  # noqa: E402
import cv2  # noqa: E402  (the shim)
from PIL import Image, ImageDraw  # noqa: E402
from zombsole.renderer import OpencvRenderer  # noqa: E402
from zombsole.things import Box, Wall, Zombie, ObjectiveLocation, DeadBody  # noqa: E402

from libzombsole_amd import render as R  # noqa: E402  (names and order of the shapes and colours only)

# name, surface, stream, kwargs, seeds, calls, full_obs_calls, max_steps: two seeds x 40 calls each
CONFIGS = [
    # the 9 x 7 generated field of obs_shapes.py (walls, boxes, objectives) with a yellow bot; 270-byte pixel rows
    ("render_field9x7_bot", "single", "discrete",
     dict(rules_name="extermination", player_names=["sniper"], map_name="field9x7", agent_id="0", initial_zombies=6,
          minimum_zombies=2, observation_scope="world", observation_position_encoding="simple"), [0, 1], 40, 1, 12),
    # bridge with four agents, a cyan bot and a zombie minimum: bodies of three colours, respawns, as views_*
    ("render_bridge_a4_bot", "multi", "rich",
     dict(rules_name="extermination", player_names=["terminator"], map_name="bridge", agent_ids=["0", "1", "2", "3"],
          initial_zombies=20, minimum_zombies=15, agent_weapons=["shotgun", "rifle", "axe", "gun"]), [31, 32], 40, 1, 0),
    # an 8-wide safehouse map: objectives, bodies on them, a crowd of zombies around two agents
    ("render_safe_crowd_a2", "multi", "discrete",
     dict(rules_name="safehouse", player_names=["randoman"], map_name="safe_crowd", agent_ids=["0", "1"],
          initial_zombies=4, minimum_zombies=4), [0, 4], 40, 1, 0),
]
FULL_FRAMES = (0, 17, 39)  # the calls of the first seed recorded as full frames


def draw(world, players):
    """The reference's frame of `world`, cropped to the map area: uint8 [10 H, 10 W, 3] RGB."""
    shown = []
    cv2.imshow = lambda _name, bgr: shown.append(np.asarray(bgr))
    W, H = world.size
    OpencvRenderer(W, H + 2 + len(players)).render(world, players)
    assert len(shown) == 1
    return np.ascontiguousarray(shown[0][:10 * H, :10 * W, ::-1])  # BGR -> RGB


def record_atlas():
    r = OpencvRenderer(3, 3)
    things = (("solid", Wall((1, 1))), ("box", Box((1, 1))), ("disc", Zombie((1, 1))), ("frame", ObjectiveLocation((1, 1))),
              ("body", DeadBody("x", "red", (1, 1))))
    masks, colors = {}, {}
    for name, th in things:
        im = Image.new("RGB", (30, 30), "black")
        r._render_thing(ImageDraw.Draw(im), 1, 1, th)
        a = np.array(im)
        m = a.any(axis=2)
        assert not m[:10].any() and not m[21:].any() and not m[:, :10].any() and not m[:, 21:].any(), name
        assert len({tuple(int(v) for v in p) for p in a[m]}) == 1, name
        masks[name] = ["".join("#" if v else "." for v in row) for row in m[10:21, 10:21]]
        colors[th.color] = [int(v) for v in a[m][0]]
    for cname in R.COLOR_NAMES:  # the colours no thing above has: drawn as a body of that colour
        if cname not in colors:
            im = Image.new("RGB", (30, 30), "black")
            r._render_thing(ImageDraw.Draw(im), 1, 1, DeadBody("x", cname, (1, 1)))
            a = np.array(im)
            colors[cname] = [int(v) for v in a[a.any(axis=2)][0]]
    return {"masks": masks, "colors": colors, "pixels": {k: sum(row.count("#") for row in v) for k, v in masks.items()}}


def main():
    only = set(sys.argv[1:])
    if not only or "atlas" in only:
        with open(os.path.join(HERE, "render_atlas.json"), "w", encoding="utf-8") as f:
            json.dump(record_atlas(), f, indent=1, sort_keys=True)
            f.write("\n")
    atlas = json.load(open(os.path.join(HERE, "render_atlas.json"), encoding="utf-8"))
    index_of = {tuple(atlas["colors"][n]): i for i, n in enumerate(R.COLOR_NAMES)}
    for cfg in CONFIGS:
        if only and cfg[0] not in only:
            continue
        side = []
        orig = golden_driver.canonical_state

        def capture(game, obstacles, K):  # run_config calls canonical_state once per recorded call, last
            frame = draw(game.world, list(game.players) + list(getattr(game, "agents", [])))
            bodies = [[p[0], p[1], R.COLOR_NAMES.index(d.color)] for p, d in game.world.decoration.items()
                      if isinstance(d, DeadBody)]
            side.append((frame, bodies))
            return orig(game, obstacles, K)

        golden_driver.canonical_state = capture
        try:
            data = golden_driver.run_config(cfg, make_golden.K)
        finally:
            golden_driver.canonical_state = orig
        it = iter(side)
        for ri, run in enumerate(data["runs"]):
            run["render"] = []
            for ci in range(len(run["calls"])):
                frame, bodies = next(it)
                rr = {"hash": hashlib.sha256(frame.tobytes()).hexdigest()[:16], "bodies": bodies}
                run["render"].append(rr)
                if ri == 0 and ci in FULL_FRAMES:
                    idx = np.full(frame.shape[:2], 255, dtype=np.uint8)
                    for rgb, i in index_of.items():
                        idx[(frame == np.array(rgb, dtype=np.uint8)).all(axis=2)] = i
                    assert ((idx != 255) == frame.any(axis=2)).all(), "a colour outside the palette"
                    rr["frame"] = base64.b64encode(zlib.compress(idx.tobytes(), 9)).decode("ascii")
        assert next(it, None) is None
        path = os.path.join(HERE, cfg[0] + ".json.gz")
        with gzip.open(path, "wt", encoding="utf-8") as f:
            json.dump(data, f, separators=(",", ":"))
        print("%-30s %8d bytes" % (cfg[0], os.path.getsize(path)))


if __name__ == "__main__":
    main()
