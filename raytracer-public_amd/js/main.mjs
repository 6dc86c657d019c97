// main.mjs -- the reference's src/main.js as an ES module under Node: its first two lines are src/main.js:1-2 AS WRITTEN (they resolve against
// libs/PathTracer.js and libs/Scene.js, the ES-module faces of this package), and what follows is the reference's sequence statement by statement
// (src/main.js:5-76) without the DOM: a {width, height} object for the <canvas>, a fixed camera for the FPSCamera, a fixed number of frames for
// requestAnimationFrame, the BVH2 dump written to data/BVH2.bin instead of POSTed to /api/write.  (No top-level await: Node 12.)
//   node raytracer-public_amd/js/main.mjs [--frames N] [--width W --height H] [--glb path] [--tris N] [--mode 0|1|2 --spp S --bounces B --seed K]
//        [--cam x,y,z --quat x,y,z,w] [--bvh2 data/BVH2.bin] [--dump data/BVH2.bin | --dump none] [--radiance frame.f32 --triangles tris.f32]
//        [--accel 0|1|2]   tree quality of buildBVH (this build's extension; 0 = the reference's tree)
//        [--animate AMP]   displace the scene before every render() and refit the tree in place (updateTriangles; tools/README.md has the formula)
// A GLB that exists and cannot be read ends the process with a non-zero status (the reference has no catch, src/main.js:20-23); only a file that
// is not there falls back to the procedural stand-in.
import * as PT from "./libs/PathTracer.js";
import * as PTScene from "./libs/Scene.js";
import fs from "fs";
import path from "path";

function arg(name, dflt) { const i = process.argv.indexOf("--" + name); return i >= 0 && i + 1 < process.argv.length ? process.argv[i + 1] : dflt; }

async function main() {
  const canvas = { width: Number(arg("width", 1920)), height: Number(arg("height", 1080)) };        // index.html:10
  const pathTracer = new PT.PathTracer(canvas, { mode: Number(arg("mode", PT.MODE_REFERENCE)), spp: Number(arg("spp", 4)), maxBounces: Number(arg("bounces", 8)), seed: Number(arg("seed", 1)), accel: Number(arg("accel", 0)) });   // src/main.js:8 (options: this build's extension)
  const camera = { position: arg("cam", "0,0,2.5").split(",").map(Number), rotation: arg("quat", "0,0,0,1").split(",").map(Number) };   // src/main.js:10-14

  await pathTracer.initialize();                                                                     // src/main.js:16

  // ---------- Scene ----------  src/main.js:18-24
  const scene = new PTScene.Scene();
  const glb = arg("glb", "/assets/dragon.glb");
  const tLoad = Date.now();
  try {
    await scene.loadGLB(glb, { normalize: true, mode: "cube" });
    console.log("Loaded", glb, "->", scene.getTriangles().length, "triangles in", Date.now() - tLoad, "ms");
  } catch (e) {
    // The reference has no catch here (src/main.js:20-23; Scene.js:27-30 rejects): a GLB that cannot be read stops the app, and so it does here.
    // The one exception is a file that is NOT THERE -- the reference's dragon.glb is not shipped (SURVEY.md 0.3) -- for which a procedural
    // dragon-class mesh of the same triangle budget stands in, and the log says so.
    if (!e || e.code !== "ENOENT") throw e;
    const n = Number(arg("tris", 871414));
    console.log("GLB not available (" + glb + "): using the procedural dragon-class stand-in,", n, "triangles");
    scene.getTrianglesFloat32 = () => PT.native().proceduralScene(0, n, 20260109);
  }
  const prebuilt = arg("bvh2", null);             // a BVH2 dumped by an earlier run (data/BVH2.bin): installed instead of rebuilding
  if (prebuilt) {
    const t0 = Date.now();
    await pathTracer.setSceneWithBVH2(scene, PT.native().readU32File(prebuilt));
    console.log("Installed prebuilt BVH2", prebuilt, "in", Date.now() - t0, "ms");
  } else await pathTracer.setScene(scene);

  // ---------- BVH Dump (ONCE) ----------  src/main.js:26-46
  const numTris = (pathTracer.trianglesData.length / 9) | 0;
  const { bytes: bvh2Bytes } = pathTracer.computeBVH2Sizing(numTris);
  const bvh2U32 = await pathTracer.readBVH2(bvh2Bytes);
  const dump = arg("dump", path.join("data", "BVH2.bin"));
  console.log("Uploading BVH2:", bvh2U32.length * 4, "bytes");
  if (dump !== "none") {
    fs.mkdirSync(path.dirname(dump), { recursive: true });
    PT.native().writeU32File(dump, bvh2U32);
  }
  console.log("BVH2 dump complete");

  // ---------- Render Loop ----------  src/main.js:48-76
  const frames = Number(arg("frames", 30));
  let frameIndex = 0;
  const animate = Number(arg("animate", 0));                  // --animate AMP: the scene as built, displaced by the wave of the frame count before every render()
  const baseTriangles = animate ? Float32Array.from(pathTracer.trianglesData) : null, movedTriangles = animate ? new Float32Array(baseTriangles.length) : null;
  const t0 = Date.now();
  for (let f = 0; f < frames; f++) {
    frameIndex++;
    pathTracer.setCameraPosition(camera.position[0], camera.position[1], camera.position[2]);
    pathTracer.setCameraQuaternion(camera.rotation[0], camera.rotation[1], camera.rotation[2], camera.rotation[3]);
    pathTracer.setFrameCount(frameIndex);
    if (animate) pathTracer.updateTriangles(PT.animateWave(baseTriangles, animate, frameIndex, movedTriangles));   // new vertices, the same tree: refit in place
    await pathTracer.render();
  }
  pathTracer.synchronize();
  console.log((frames / ((Date.now() - t0) / 1000)).toFixed(1) + " FPS (" + frames + " frames)");
  const radiance = arg("radiance", null), trisOut = arg("triangles", null);      // what a test compares with the oracle: the last frame (f32 RGBA) and the triangles it was traced over
  if (radiance) { const img = pathTracer.readRadiance(); fs.writeFileSync(radiance, Buffer.from(img.buffer, img.byteOffset, img.byteLength)); }
  if (trisOut) { const t = pathTracer.trianglesData; fs.writeFileSync(trisOut, Buffer.from(t.buffer, t.byteOffset, t.byteLength)); }
  pathTracer.destroy();
}

main().catch((e) => { console.error(e); process.exit(1); });
