// worker_threads counterpart of the reference's Web Worker (js/planet-worker.js) for the part of its message protocol
// that is the device path: `generate` (:136-339), the retained state W (:277-292), `reapply` (:341-440), `editRecompute` (:442-577),
// `computeClimate` (:579-677) and the dispatcher (:944-954); and `exportMap`, which the reference runs on its page with WebGL
// (js/planet-mesh.js:1752-2180) and a Node host has no other way to get.
//
//   cmd 'generate' { N, P, jitter, nMag, numContinents, <the six sliders>, continentSizeVariety = 0, temperatureOffset = 0, precipitationOffset = 0,
//                    landCoverage = 0.3, seed?, toggledIndices? }   (:136-339)
//                  a seed becomes a planet, every stage native: mesh (the pole fan numbered as the reference's addPoleToMesh numbers it), neighbour
//                  distances, triangle centres, generateCoarsePlates (generatePlates + assignOceanLand on the 20 000-cell mesh: native host stages,
//                  a few milliseconds, no device part), projectCoarsePlates (device), smoothAndReconnectPlates(…, 3), the toggled plates, the three
//                  density tables, then the chain `editRecompute` runs: buildSuperPlates when P >= 8, assignElevation, runPostProcessing with the
//                  call's hotspot layer, triangle elevations — the field stays on the device from assignElevation on.  Without `seed`:
//                  Math.floor(Math.random() * 16777216).  Progress 0 / 10 / 20 / 25 / 35 / 60 / 75 with the reference's labels.  Climate is not run
//                  here, as for every other command of this worker: skipClimate is reported as true, the 19 climate fields are null and the caller
//                  follows with `computeClimate` (the reference's own behaviour above 300 k cells).  The result is the reference's `done` message
//                  (same keys in the same order, _pipelineTiming with the reference's stage names less the climate entries), the same seven
//                  buffers transferred.  W keeps what reapply, editRecompute, computeClimate and exportMap need: the pre-erosion field and the
//                  hotspot layer on the device, triangles, halfedges, r_plate, plateSeeds, plateVec, the densities, P, both ocean sets and the three
//                  climate parameters; the wind and ocean blocks are invalid, as after `retain`.  N or P not a positive integer:
//                  `generate needs N and P (a generate without them is not served by the device worker)`, the state is kept.  A failure
//                  before the projection (mesh, coarse plates) keeps the previous state too; one after it leaves no state at all.
//                  -> { type: 'done', triangles, halfedges, numRegions, r_xyz, t_xyz, r_plate, plateSeeds, plateVec, plateIsOcean, originalPlateIsOcean,
//                       plateDensity, plateDensityLand, plateDensityOcean, prePostElev, r_elevation, t_elevation, mountain_r, coastline_r, ocean_r,
//                       r_stress, <the 19 climate fields: null>, skipClimate: true, seed, nMag, debugLayers, _timing, _pipelineTiming, _postTiming,
//                       _workerTotal, _params }
//   cmd 'retain'   { mesh: { numRegions, adjOffset, adjList, triangles?, halfedges? }, r_xyz, neighborDist?, prePostElev, seed, r_hotspot?,
//                    r_plate?, plateIsOcean?, plateSeeds?, plateVec?, plateDensity?, P? }
//                  What `generate` leaves in W for later reapplies, handed over by a caller that made the planet elsewhere.  The mesh, positions and the
//                  pre-erosion field go to HBM ONCE and stay there.  r_plate (Int32Array) and plateIsOcean (the ids of the
//                  oceanic plates: a Set, an array or an Int32Array) are what a later `computeClimate` needs.  plateSeeds (the Set's
//                  iteration order: an array, a Set or an Int32Array), plateVec ({ id: { pole, omega } }), plateDensity ({ id: density })
//                  and P (the plate count asked of `generate`) are what a later `editRecompute` needs on top of them.
//                  -> { type: 'retained', numRegions }
//   cmd 'reapply'  { terrainWarp, smoothing, glacialErosion, hydraulicErosion, thermalErosion, ridgeSharpening, skipClimate? }
//                  restore the pre-erosion field on the device (no upload), runPostProcessing resident, triangle
//                  elevations; the climate stages are not run here (skipClimate is reported as true, the reference's own
//                  behaviour above 300 k cells).  Same result message as the reference, typed arrays transferred:
//                  -> { type: 'reapplyDone', skipClimate: true, r_elevation, t_elevation, erosionDelta, _reapplyTiming, _postTiming }
//   cmd 'importHeightmap' { N, jitter, grayscale, imageWidth, imageHeight, sliders, seed? }   (:771-940)
//                  the reference's handler with every stage native: mesh, neighbour distances, triangle centres, the sampler
//                  (device), runPostProcessing resident, synthetic plates and region classification (device), triangle
//                  elevations.  The sampled field is kept as W.prePostElev on the device, so a following `reapply` works on the
//                  imported planet.  Climate is not run (skipClimate is reported as true, as for reapply); the result is the
//                  reference's `done` message with the climate fields null, buffers transferred as the reference does.  Copies
//                  of r_plate and plateIsOcean stay in W with the seed, so a following `computeClimate` works as well.
//   cmd 'computeClimate' { temperatureOffset?, precipitationOffset?, landCoverage? }   (:579-677)
//                  computeWind, computeOceanCurrents, computePrecipitation, computeTemperature and classifyKoppen on the device,
//                  resident, on the planet's current elevation.  Wind and ocean are skipped while the planet's blocks belong to
//                  that elevation (the reference's cachedWind: `reapply`, `importHeightmap` and `retain` invalidate them); the
//                  parameters persist in W as getClimateParams keeps them (:104-110).  Progress labels and the result as the
//                  reference posts them:
//                  -> { type: 'climateDone', <the 19 climate fields>, climateDebugLayers, _climateTiming: { wind, ocean,
//                       precipitation, temperature, koppen, workerTotal } }
//   cmd 'editRecompute' { plateIsOcean, plateDensity, nMag, <the six sliders>, skipClimate? }   (:442-577)
//                  what the editor sends when a plate changes kind: buildSuperPlates (when W.P >= 8), assignElevation, runPostProcessing
//                  resident with the call's own hotspot layer, triangle elevations — every stage native, the field never leaves the
//                  device between them.  The new pre-erosion field becomes W.prePostElev (on the device), so a following `reapply`
//                  starts from the edited planet.  Climate is not run here (skipClimate is reported as true and the 19 climate fields
//                  are null, as for reapply); a following `computeClimate` serves it with the edited plateIsOcean.  Needs a state
//                  retained with r_plate, plateSeeds and plateVec: a state left by `importHeightmap` has synthetic plates without
//                  poles and is refused.
//                  -> { type: 'editDone', skipClimate: true, prePostElev, r_elevation, t_elevation, mountain_r, coastline_r, ocean_r,
//                       r_stress, <the 19 climate fields: null>, debugLayers, _editTiming, _timing, _postTiming }
//   cmd 'exportMap' { type | types, width, png?, layers?, centerLon? }   (js/planet-mesh.js:1752-2180; layers and centerLon: the map view, :200-382)
//                  the equirectangular map, width x width / 2, of the planet's current elevation and Koppen block in one or
//                  several of the reference's six kinds (color, heightmap, landheightmap, landmask, biome, koppen): one raster on
//                  the device, one colour pass per type, and with `png` the PNG file of each (js/map-export.js).  Needs a state
//                  retained with mesh.triangles and mesh.halfedges (importHeightmap keeps both); biome and koppen need a
//                  computeClimate before them (`no Koppen result` otherwise: the reference's silent fallback to the colour map is
//                  not offered).  Progress: `Rendering...` at 0, then 80 k / n after each type, `Encoding PNG...` at 85 with png.
//                  `layers`: names of the map view's debugLayer switch, each one more map after the types' (filename
//                  orogen-layer-<name>-<seed>.png, ours).  A climate layer (continentality, temp*, precip*, rainShadow*, oceanCurrent*,
//                  pressure*, windSpeed* with Summer / Winter) reads the block computeClimate left on the planet (`no wind result`
//                  and so on before it); any other key of the retained debugLayers (erosionDelta, hotspot, the twelve assignElevation
//                  layers, superPlates) is coloured by debugValueToColor over its own range, which is reduced on the device.
//                  `centerLon` (radians, within [-pi, pi]) draws the map around that meridian.  Progress then counts types + layers.
//                  -> { type: 'exportDone', width, height, maps: [{ type, filename, rgba, png? }],
//                       _exportTiming: { raster, color, encode, workerTotal } }, the buffers transferred
//   cmd 'renderGlobe' { type | types, layers?, width, height, camera?, shade?, rivers?, background?, exaggeration?, light?, ambient?,
//                  diffuse?, png? }   (ours: the picture the reference's page draws with three.js, without a page)
//                  -> { type: 'renderGlobeDone', width, height, covered, uncovered, maps: [{ type, filename, rgba, png? }], _exportTiming }
//                  The displaced globe of the retained planet through a camera that looks at its centre (js/view-export.js; the contract
//                  is in csrc/view_ops.h).  camera: { lon, lat, distance, fov } in degrees (north +Y, longitude 0 at +Z) or { eye, fov };
//                  fov 0 with halfHeight is orthographic; nothing: the reference's 50 degrees at (0, 0.4, 2.8).  shade (default true):
//                  one Lambert term per facet from `light` (default the reference's sun).  background: R | G << 8 | B << 16 | A << 24
//                  for the pixels nothing covers (default 0x030308 opaque, 0: transparent).  types, layers, rivers: exportMap's.
//   cmd 'exportCubeMap' { type | types, faceSize, png?, layers?, layout? }   (ours: the reference exports no cube map)
//                  the cube map of the planet's current elevation and Koppen block: six square faces of faceSize x faceSize by
//                  gnomonic projection, exactly the globe mesh seen from its centre, in the OpenGL order px nx py ny pz nz (north
//                  is +Y, longitude 0 is +Z: pz is centred on the map's centre, row 0 of the four side faces is north; the face
//                  table is in include/worogen.h).  One raster on the device (csrc/cube.hip), one colour pass per type and layer;
//                  types, layers, their needs and their checks are exportMap's, the messages name exportCubeMap.  faceSize: an
//                  integer from 1 to 16384.  `layout`: 'faces' (the default) gives six images per map, views of one buffer,
//                  filenames orogen-<stem>-<seed>-<face>.png; 'column' gives the one faceSize x 6 faceSize image with the faces
//                  stacked in that order, as a single entry { face: 'column', filename: orogen-<stem>-<seed>-column.png }.  A side
//                  that spans more than 35.26 degrees may be missing from a face (no generated mesh has one).  Progress as exportMap.
//                  -> { type: 'exportCubeDone', faceSize, maps: [{ type, faces: [{ face, filename, rgba, png? }] }],
//                       _exportTiming: { raster, color, encode, workerTotal } }, the buffers transferred
//   cmd 'exportRelief' { projection?, width | faceSize, centerLon?, kinds, strength?, flatOcean?, layout?, png? }   (ours: the reference exports no relief)
//                  the relief of the planet's current elevation (js/relief-export.js; csrc/relief.hip): the globe mesh's own flat
//                  triangles sampled at every pixel centre, so heights vary inside a region.  `projection`: 'map' (the default;
//                  width x width / 2 around `centerLon`) or 'cube' (six faces of faceSize, `layout` as for exportCubeMap).  `kinds`:
//                  some of height16, landHeight16 (16-bit grey, linear in the reference's heightmap / land-heightmap shade, no gamma:
//                  Uint16Array), normal, normalObject (RGBA8 normals in tangent / object space of the surface displaced as the globe
//                  is, times `strength`, default 1; `flatOcean`: elevations <= 0 count as 0: Uint8ClampedArray).  With `png` every
//                  image comes with its file: 16-bit greyscale PNGs for the first two.  Filenames orogen-<kind>-<seed>.png and
//                  orogen-cube-<kind>-<face>-<seed>.png.  Needs what exportMap needs of the retained state.  The relief raster leaves
//                  the same region map as exportMap's, so the planet stays paintable.
//                  -> { type: 'exportReliefDone', projection, width, height | faceSize, covered, uncovered,
//                       maps: [{ kind, filename, data, png? }] | [{ kind, faces: [{ face, filename, kind, data, png? }] }],
//                       _exportTiming: { render, encode, workerTotal } }, the buffers transferred
//   cmd 'exportGlobe' { view?, layer?, plates?, wireframe?, superPlateBorders?, glb?, windArrows?, oceanCurrentArrows?, itcz?, grid?, rivers? }   (js/planet-mesh.js:620-836, :533-576)
//                  the globe mesh three.js would draw, of the planet's current elevation: one displaced triangle per side, nine floats
//                  of positions and nine of colours each, built on the device (js/globe-export.js).  `view`: color (the default),
//                  heightmap, landheightmap, biome or koppen; `layer`: a layer as for exportMap, a climate layer from the planet's
//                  block or a key of the retained debugLayers; `plates`: the plate colours (computePlateColors over the retained
//                  plateSeeds and plateIsOcean, needs r_plate).  `wireframe` adds the Voronoi wireframe, `superPlateBorders` the
//                  borders of the retained debugLayers.superPlates (true) or of a Float32Array of the caller's.  With `glb` the answer carries the binary glTF file of all of it
//                  instead of the arrays.  Needs what exportMap needs of the retained state and answers as it does without it.
//                  `windArrows`, `oceanCurrentArrows`, `itcz`: 'summer' | 'winter', `grid`: degrees add the globe form of that overlay (see
//                  exportOverlays) as arrays (arrows: { position, color }) or as LINES primitives of the GLB.
//                  Progress: `Building globe...` at 0, `Done` at 90.
//                  -> { type: 'globeDone', view, filename, numSides, bounds, glb | position, color[, wireframe][, superPlateBorders][, windArrows]
//                       [, oceanCurrentArrows][, itcz][, grid][, rivers][, outlines],
//                       _globeTiming: { workerTotal } }, the buffers transferred
//   cmd 'computeRivers' { runoff?, download? }   (ours: js/rivers.js, csrc/rivers.hip)
//                  the rivers and lakes of the planet's current elevation: every land cell drains to its lowest neighbour, depressions
//                  spill over their lowest pass so that rivers reach the sea, and the runoff is accumulated down the receivers.
//                  `runoff`: 'precip' (the default: the mean of the two precipitation fields computeClimate left on the planet; `no
//                  precipitation result` before it), 'uniform' (1 per land cell, needs no climate) or a Float32Array of numRegions
//                  values.  The five fields stay on the planet for the `rivers` option of exportMap, exportCubeMap and exportGlobe,
//                  until the next computeRivers; they describe the elevation of that moment.  With `download` they come back too.
//                  -> { type: 'riversDone', landCells, pits, spilledBasins, endorheicBasins, lakeCells, rounds, launches
//                       [, r_river_receiver, r_river_basin: Int32Array, r_lake_level, r_river_flow: Float32Array, r_river_discharge: BigUint64Array],
//                       _riversTiming: { workerTotal } }, the buffers transferred
//                  exportMap and exportCubeMap take `rivers: { minFlow }`: the types' maps (not the layers') get the river cells whose flow
//                  reaches minFlow and the lakes painted (41, 98, 168); exportGlobe takes the same and adds the river segments as `rivers`
//                  (Float32Array, six floats each) or as one more LINES primitive of the GLB.  `no rivers result` before computeRivers.
//   cmd 'exportOutlines' { source, levels?, values?, onlyClass?, format?, width?, centerLon? }   (ours: js/outline-export.js, csrc/outline.hip)
//                  the line where one class of cells ends and another begins, traced on the device into ordered closed rings of the
//                  Voronoi cells' sides.  `source`: 'coast' (elevation > 0 of the planet's current field), 'lakes' (the lake levels of
//                  computeRivers; `no rivers result` before it), 'koppen' (computeClimate's classes; `no Koppen result` before it),
//                  'levels' with `levels`: up to 32 ascending elevations, 'values' with `values`: an Int32Array of numRegions classes,
//                  and the shorthands 'plates' (the retained r_plate) and 'superPlates' (the retained debugLayers.superPlates, a NaN
//                  cell a class of its own).  `onlyClass`: the rings of that class alone (default: of every class, every boundary
//                  edge then once per class).  `format`: 'arrays' (the default), 'geojson' or 'svg' (`width`, default 2048, and
//                  `centerLon` in radians: exportMap's pixel frame); both texts are cut where a ring crosses the map's edge.
//                  Needs what exportMap needs of the retained state.
//                  -> { type: 'outlinesDone', source, format, filename, boundarySides, rings, longestRing, rounds, launches,
//                       sides, ring_start, ring_class, ring_of_side: Int32Array, lonlat: Float64Array (radians) | text,
//                       _outlineTiming: { workerTotal } }, the buffers transferred
//                  exportGlobe takes `outlines: { source, levels?, values?, onlyClass? }` and adds the rings, displaced as the super-plate
//                  borders are (base 1.002), as `outlines` (Float32Array, six floats per segment) or as one more LINES primitive of the GLB.
//   cmd 'exportOverlays' { windArrows?, oceanCurrentArrows?, itcz?, grid?, centerLon? }   (js/planet-mesh.js:1289-1749, :385-469)
//                  the line overlays of the reference's views in both forms, globe and map (js/overlay-export.js): `windArrows`,
//                  `oceanCurrentArrows`: 'summer' | 'winter', the arrows of that season from the blocks computeClimate left on the planet,
//                  built on the device (`no wind result` / `no ocean result` before it); `itcz`: 'summer' | 'winter', the green line of
//                  the pressure views from the cached wind result; `grid`: the spacing of the latitude / longitude grid in degrees.
//                  `centerLon` (radians) is the map view's centre meridian; the map form of the ITCZ line ignores it, as the reference does.
//                  -> { type: 'overlaysDone', centerLon[, windArrows, oceanCurrentArrows: { globe: { position, color }, map: { position, color }, count }]
//                       [, itcz, grid: { globe, map }], _overlayTiming: { workerTotal } }, the buffers transferred
//   cmd 'pick' { directions | rays | map: { points, centerLon? } }   (js/edit-mode.js:18-93)
//                  the editor's hit test on the retained planet (js/edit-mode.js here, csrc/pick.hip): which region, and so which
//                  plate, lies under a pointer.  `directions`: three numbers per query, findNearestRegion itself; `rays`: six per
//                  query, origin and normalised direction of the ray in the planet's local space (getHitInfoGlobe's arithmetic: the
//                  sphere of radius 1.08); `map`: `points` wx, wy per query on the map plane around `centerLon` (getHitInfoMap's).
//                  Exactly one of the three; at most 65536 queries.
//                  -> { type: 'picked', regions: Int32Array (-1: no region), plates: Int32Array (-1: no region or no retained r_plate) }
//   cmd 'setHighlight' { pendingToggles?, hoveredPlate?, hoveredKoppen? }   (js/planet-mesh.js:953-1244)
//                  the editor state the reference's page keeps: the plates queued for a rebuild (tinted green where the plate is ocean
//                  now, blue where it is land, by the retained plateIsOcean), the hovered plate and the hovered Koppen class
//                  (brightened; the class needs computeClimate's Koppen result).  Uses the retained r_plate.  exportGlobe and exportMap
//                  then show the tints with no further option, until the state is replaced or cleared: an empty request clears it,
//                  and so do editRecompute (the reference clears pendingToggles after a rebuild), importHeightmap, generate, retain and
//                  dispose, which replace the planet.
//                  -> { type: 'highlightSet', cleared, counts: { pendingOcean, pendingLand, hoveredPlate, hoveredKoppen } }
//   cmd 'dispose'  frees the retained state -> { type: 'disposed' }
//   progress / errors exactly as the reference posts them: { type: 'progress', pct, label }, { type: 'error', message, stack };
//   an unknown command answers `Unknown command: <cmd>` (:952).
//
// Usage (Node >= 12):  const w = new Worker(new URL('./planet-worker.js', import.meta.url)); w.postMessage({ cmd: 'retain', ... })
import { parentPort } from 'worker_threads';
import { performance } from 'perf_hooks';
import addon, { defaultContext } from './native.js';
import { runPostProcessingResident } from './post-processing.js';
import { buildSphere, computeNeighborDist, generateTriangleCenters } from './sphere-mesh.js';
import { platesFromDevice } from './heightmap-import.js';
import { OCEAN_KEYS, PRECIP_KEYS, TEMP_KEYS, downloadAll } from './climate-blocks.js';
import { denseTable, plateDensities, LAYERS } from './plate-table.js';
import { generateCoarsePlates } from './coarse-plates.js';
import { SimplexNoise } from './simplex-noise.js';
import { MAP_TYPES, MAP_LAYERS, CUBE_MAX_FACE_SIZE, exportFilename, layerFilename, cubeFilename, cubeFaces, encodePng, rasterOnPlanet } from './map-export.js';
import { VIEW_MAX_SIZE, viewFilename, viewParams } from './view-export.js';
import { RELIEF_KINDS, reliefIs16, reliefFilename, reliefFaces, exportReliefOnPlanet, exportCubeReliefOnPlanet, encodePng16 } from './relief-export.js';
import { GLOBE_PLATES, GLOBE_TYPE_VIEWS, computePlateColors, exportGlobeOnPlanet, globeFilename } from './globe-export.js';
import { findNearestRegions, hitDirectionsGlobe, hitDirectionsMap, setHighlight, clearHighlight, PICK_MAX_QUERIES } from './edit-mode.js';
import { computeRiversOnPlanet, checkedMinFlow, RIVER_KEYS } from './rivers.js';
import { OUTLINE_FIELDS, OUTLINE_SOURCES, buildOutlineOnPlanet, outlineFilename, outlineToGeoJSON, outlineToSvg } from './outline-export.js';
import { SEASONS, windArrowsOnPlanet, oceanCurrentArrowsOnPlanet, itczLine, grids } from './overlay-export.js';

let W = null;          // retained state (js/planet-worker.js:22)

function progress(pct, label) { parentPort.postMessage({ type: 'progress', pct, label }); }

// the retained planet holds several GB of device memory at 40 M cells and its JS handle is a few bytes: free it explicitly
function releaseRetained() { if (W && W.planet) addon.planetDestroy(W.planet); W = null; }

function handleRetain(data) {
    try {
        const { mesh, r_xyz, neighborDist, prePostElev, seed, r_hotspot, r_plate, plateIsOcean, plateSeeds, plateVec, plateDensity, P } = data;
        if (!mesh || !(mesh.adjOffset instanceof Int32Array) || !(mesh.adjList instanceof Int32Array)) throw new TypeError('retain: mesh.adjOffset / mesh.adjList must be Int32Arrays');
        if (!(r_xyz instanceof Float32Array) || !(prePostElev instanceof Float32Array)) throw new TypeError('retain: r_xyz and prePostElev must be Float32Arrays');
        if (r_plate !== undefined && r_plate !== null && (!(r_plate instanceof Int32Array) || r_plate.length !== mesh.numRegions)) throw new TypeError('retain: r_plate must be an Int32Array of numRegions entries');
        releaseRetained();                               // a second retain replaces the first: its device memory goes now, not at the next GC
        const planet = addon.planetCreate(defaultContext(), mesh.numRegions, mesh.adjOffset, mesh.adjList, r_xyz, neighborDist || null);
        addon.planetUpload(planet, prePostElev, null);
        if (r_hotspot) addon.planetUploadHotspot(planet, r_hotspot);
        addon.planetSaveState(planet);                  // W.prePostElev, device copy
        W = { planet, numRegions: mesh.numRegions, triangles: mesh.triangles || null, halfedges: mesh.halfedges || null, seed, hasHotspot: !!r_hotspot,
              r_plate: r_plate || null, plateIsOcean: (plateIsOcean !== undefined && plateIsOcean !== null) ? Int32Array.from(plateIsOcean) : null,
              plateSeeds: (plateSeeds !== undefined && plateSeeds !== null) ? Int32Array.from(plateSeeds) : null, plateVec: plateVec || null,
              plateDensity: Object.assign({}, plateDensity || {}), P: P || 0, cachedWind: null, cachedOcean: null };
        parentPort.postMessage({ type: 'retained', numRegions: mesh.numRegions });
    } catch (err) {
        parentPort.postMessage({ type: 'error', message: err.message, stack: err.stack });
    }
}

function handleReapply(data) {
    if (!W) { parentPort.postMessage({ type: 'error', message: 'No retained state for reapply' }); return; }
    try {
        const tTotal0 = performance.now();
        progress(0, 'Reapplying terrain…');
        let t0 = performance.now();
        W.cachedWind = null; W.cachedOcean = null;     // the elevation changes: the wind and ocean blocks no longer belong to it
        addon.planetRestoreState(W.planet);             // r_elevation = new Float32Array(W.prePostElev), on the device
        const r_elevation = new Float32Array(W.numRegions);
        const tClone = performance.now() - t0;

        progress(20, 'Eroding terrain…');
        t0 = performance.now();
        const { dl_erosionDelta, postTiming } = runPostProcessingResident(W.planet, W.numRegions, r_elevation, data, W.seed, W.hasHotspot);
        const tPost = performance.now() - t0;

        progress(70, 'Computing triangle elevations…');
        t0 = performance.now();
        const t_elevation = W.triangles ? addon.triangleElevations(W.triangles, r_elevation) : new Float32Array(0);
        const tTriElev = performance.now() - t0;

        const result = {
            type: 'reapplyDone',
            skipClimate: true,
            r_elevation,
            t_elevation,
            erosionDelta: dl_erosionDelta,
            _reapplyTiming: { clone: tClone, postProcessing: tPost, wind: 0, ocean: 0, precipitation: 0, temperature: 0,
                              triangleElevations: tTriElev, workerTotal: performance.now() - tTotal0 },
            _postTiming: postTiming
        };
        if (W.debugLayers) W.debugLayers = { ...W.debugLayers, erosionDelta: new Float32Array(dl_erosionDelta) };     // a copy: the buffer leaves with the message
        parentPort.postMessage(result, [r_elevation.buffer, t_elevation.buffer, dl_erosionDelta.buffer]);
    } catch (err) {
        parentPort.postMessage({ type: 'error', message: err.message, stack: err.stack });
    }
}

const CLIMATE_NULLS = ['r_wind_east_summer', 'r_wind_north_summer', 'r_wind_east_winter', 'r_wind_north_winter', 'itczLons', 'itczLatsSummer',
    'itczLatsWinter', 'r_ocean_current_east_summer', 'r_ocean_current_north_summer', 'r_ocean_current_east_winter', 'r_ocean_current_north_winter',
    'r_ocean_speed_summer', 'r_ocean_speed_winter', 'r_ocean_warmth_summer', 'r_ocean_warmth_winter', 'r_precip_summer', 'r_precip_winter',
    'r_temperature_summer', 'r_temperature_winter'];           // buildClimateFields(null, ...) (:112-134)

function handleImportHeightmap(data) {
    const { N, jitter, grayscale, imageWidth, imageHeight, smoothing, hydraulicErosion, thermalErosion, ridgeSharpening, glacialErosion, terrainWarp, seed: overrideSeed } = data;
    const timing = [];
    try {
        if (!(grayscale instanceof Uint8Array) && !(grayscale instanceof Uint8ClampedArray)) throw new TypeError('importHeightmap: grayscale must be a Uint8Array or Uint8ClampedArray');
        if (!(imageWidth >= 1 && imageHeight >= 1) || grayscale.length !== imageWidth * imageHeight) throw new RangeError('importHeightmap: grayscale length must be imageWidth*imageHeight');
        const tTotal0 = performance.now();
        progress(0, 'Building sphere mesh\u2026');
        const seed = (overrideSeed !== undefined && overrideSeed !== null) ? overrideSeed : Math.floor(Math.random() * 16777216);
        let t0 = performance.now();
        const built = buildSphere(N, jitter, seed, false, (data.deviceMesh || data.devicePoints) ? defaultContext() : null, !!data.devicePoints);      // deviceMesh: the device builder, the same arrays; devicePoints: the points from the device too
        const { mesh, r_xyz } = built;
        timing.push({ stage: 'Sphere mesh', ms: performance.now() - t0 });
        t0 = performance.now();
        const neighborDist = built.neighborDist || computeNeighborDist(mesh, r_xyz);
        timing.push({ stage: 'Neighbor distances', ms: performance.now() - t0 });
        t0 = performance.now();
        const t_xyz = generateTriangleCenters(mesh, r_xyz);
        timing.push({ stage: 'Triangle centers', ms: performance.now() - t0 });

        progress(20, 'Sampling heightmap\u2026');
        t0 = performance.now();
        releaseRetained();
        const planet = addon.planetCreate(defaultContext(), mesh.numRegions, mesh.adjOffset, mesh.adjList, r_xyz, neighborDist);
        W = { planet, numRegions: mesh.numRegions, triangles: mesh.triangles, halfedges: mesh.halfedges, seed, hasHotspot: false, r_plate: null, plateIsOcean: null,
              plateSeeds: null, plateVec: null, plateDensity: {}, P: 0, cachedWind: null, cachedOcean: null };
        const prePostElev = addon.sampleHeightmap(planet, grayscale, imageWidth, imageHeight, true);
        addon.planetSaveState(planet);                  // W.prePostElev, device copy
        timing.push({ stage: 'Sample heightmap', ms: performance.now() - t0 });

        progress(35, 'Processing terrain\u2026');
        t0 = performance.now();
        const r_elevation = new Float32Array(mesh.numRegions);
        const { dl_erosionDelta, postTiming } = runPostProcessingResident(planet, mesh.numRegions, r_elevation,
            { smoothing, glacialErosion, hydraulicErosion, thermalErosion, ridgeSharpening, terrainWarp }, seed, false);
        timing.push({ stage: 'Terrain post-processing', ms: performance.now() - t0 });

        progress(50, 'Deriving plates\u2026');
        t0 = performance.now();
        const { r_plate, plateSeeds, plateIsOcean, plateVec } = platesFromDevice(addon.syntheticPlates(planet));
        timing.push({ stage: 'Synthetic plates', ms: performance.now() - t0 });
        const regions = addon.classifyRegions(planet);
        W.r_plate = new Int32Array(r_plate); W.plateIsOcean = Int32Array.from(plateIsOcean);     // copies: r_plate's buffer leaves with the message
        W.debugLayers = { erosionDelta: dl_erosionDelta };                                     // stays here: the message clones it
        W.syntheticSeeds = Int32Array.from(plateSeeds);  // for exportGlobe's plate view only: W.plateSeeds stays null, editRecompute refuses synthetic plates

        progress(75, 'Computing triangle elevations\u2026');
        t0 = performance.now();
        const t_elevation = addon.triangleElevations(mesh.triangles, r_elevation);
        timing.push({ stage: 'Triangle elevations', ms: performance.now() - t0 });
        t0 = performance.now();
        const r_stress = new Float32Array(mesh.numRegions);
        timing.push({ stage: 'Clone state for retention', ms: performance.now() - t0 });

        const climate = {};
        for (const k of CLIMATE_NULLS) climate[k] = null;
        const result = {
            type: 'done', triangles: mesh.triangles, halfedges: mesh.halfedges, numRegions: mesh.numRegions, r_xyz, t_xyz, r_plate,
            plateSeeds: Array.from(plateSeeds), plateVec, plateIsOcean: Array.from(plateIsOcean), originalPlateIsOcean: Array.from(plateIsOcean),
            plateDensity: {}, plateDensityLand: {}, plateDensityOcean: {}, prePostElev, r_elevation, t_elevation,
            mountain_r: Array.from(regions.mountain_r), coastline_r: Array.from(regions.coastline_r), ocean_r: Array.from(regions.ocean_r),
            r_stress, ...climate, skipClimate: true, seed, nMag: 0, debugLayers: { erosionDelta: dl_erosionDelta },
            _timing: [], _pipelineTiming: timing, _postTiming: postTiming, _workerTotal: performance.now() - tTotal0,
            _params: { N, P: 0, jitter, nMag: 0, numContinents: 0, smoothing, terrainWarp, hydraulicErosion, thermalErosion, ridgeSharpening, glacialErosion, seed }
        };
        parentPort.postMessage(result, [r_xyz.buffer, t_xyz.buffer, r_plate.buffer, prePostElev.buffer, r_elevation.buffer, t_elevation.buffer, r_stress.buffer]);
    } catch (err) {
        parentPort.postMessage({ type: 'error', message: err.message, stack: err.stack });
    }
}

// addon.buildSuperPlates' result as the dense table addon.assignElevation takes for its super plates (ids 0 .. n - 1, all with a vector)
function superPlateTable(res) {
    const n = res.numSuperPlates;
    return { numIds: n, hasVec: new Uint8Array(n).fill(1), pole: res.pole, omega: res.omega, isOcean: res.isOcean, density: res.density };
}

// The part `generate` (:203-273) and `editRecompute` (:459-480) have in common, every stage native on W.planet: buildSuperPlates when
// W.P >= 8, assignElevation, runPostProcessing with the call's own hotspot layer, triangle elevations.  assignElevation leaves the field
// resident; it is saved there as the new W.prePostElev and never leaves the device before the post-processing has run.
// onStage(name) is called before 'elevation', 'erosion' and 'triangles' (the callers post their own progress labels).
function elevationChain(sliders, nMag, onStage) {
    const { planet, numRegions: N, r_plate, plateSeeds, plateVec, seed } = W;
    const spread = 5;
    const plates = denseTable(W.plateIsOcean, plateVec, W.plateDensity, plateSeeds);

    let t0 = performance.now();
    let sup = null;
    if ((W.P || 0) >= 8) sup = addon.buildSuperPlates(planet, r_plate, plates, plateSeeds);
    const tSuper = performance.now() - t0;

    onStage('elevation');
    t0 = performance.now();
    if (!W.noise) W.noise = new SimplexNoise(seed);
    const res = addon.assignElevation(planet, r_plate, plates, plateSeeds, sup ? sup.r_superPlate : null, sup ? superPlateTable(sup) : null,
                                      W.noise.perm, W.noise.pm12, nMag, seed, spread, true);
    const _timing = addon.lastStageTiming(planet);
    const tElev = performance.now() - t0;
    const debugLayers = {};
    LAYERS.forEach((name, i) => { debugLayers[name] = res.debugLayers.subarray(i * N, (i + 1) * N); });
    if (sup) debugLayers.superPlates = new Float32Array(sup.r_superPlate);
    const prePostElev = res.r_elevation;

    onStage('erosion');
    t0 = performance.now();
    W.cachedWind = null; W.cachedOcean = null;     // the elevation changes: the wind and ocean blocks no longer belong to it
    addon.planetSaveState(planet);                  // the new W.prePostElev, device copy: assignElevation left the field resident
    addon.planetUploadHotspot(planet, debugLayers.hotspot);
    const r_elevation = new Float32Array(N);
    const { dl_erosionDelta, postTiming } = runPostProcessingResident(planet, N, r_elevation, sliders, seed, true);
    const tPost = performance.now() - t0;
    debugLayers.erosionDelta = dl_erosionDelta;

    onStage('triangles');
    t0 = performance.now();
    const t_elevation = W.triangles ? addon.triangleElevations(W.triangles, r_elevation) : new Float32Array(0);
    const tTriElev = performance.now() - t0;
    return { sup, res, _timing, debugLayers, prePostElev, r_elevation, t_elevation, postTiming, tSuper, tElev, tPost, tTriElev };
}

// js/planet-worker.js:442-577 with every stage native, on W.planet
function handleEditRecompute(data) {
    if (!W) { parentPort.postMessage({ type: 'error', message: 'No retained state for editRecompute (not served by the device worker before retain)' }); return; }
    const missing = ['r_plate', 'plateSeeds', 'plateVec'].filter((k) => !W[k]);
    if (missing.length) {
        parentPort.postMessage({ type: 'error', message: `editRecompute: the retained state has no ${missing.join(' and ')} (pass them to retain; the synthetic plates of importHeightmap have no poles, and edits of an imported planet are not served)` });
        return;
    }
    getClimateParams(data);                              // the parameters persist in W for the computeClimate that follows (:446)
    try {
        const tTotal0 = performance.now();
        progress(0, 'Rebuilding elevation…');
        clearHighlight(W.planet);                        // the reference clears pendingToggles after a rebuild
        W.plateIsOcean = Int32Array.from(data.plateIsOcean);
        W.plateDensity = Object.assign({}, data.plateDensity);
        const c = elevationChain(data, data.nMag, (stage) => {
            if (stage === 'erosion') progress(50, 'Eroding terrain…');
            else if (stage === 'triangles') progress(75, 'Computing triangle elevations…');
        });
        W.debugLayers = c.debugLayers;                    // what exportMap's generic layers read; the message clones them

        const climate = {};
        for (const k of CLIMATE_NULLS) climate[k] = null;
        const result = {
            type: 'editDone', skipClimate: true, prePostElev: c.prePostElev, r_elevation: c.r_elevation, t_elevation: c.t_elevation,
            mountain_r: Array.from(c.res.mountain), coastline_r: Array.from(c.res.coastline), ocean_r: Array.from(c.res.ocean), r_stress: c.res.r_stress,
            ...climate, debugLayers: c.debugLayers,
            _editTiming: { elevation: c.tElev, postProcessing: c.tPost, wind: 0, ocean: 0, precipitation: 0, temperature: 0, triangleElevations: c.tTriElev,
                           retainState: 0, workerTotal: performance.now() - tTotal0 },
            _timing: c._timing, _postTiming: c.postTiming
        };
        parentPort.postMessage(result, [c.prePostElev.buffer, c.r_elevation.buffer, c.t_elevation.buffer, c.res.r_stress.buffer]);
    } catch (err) {
        parentPort.postMessage({ type: 'error', message: err.message, stack: err.stack });
    }
}

// js/planet-worker.js:136-339 with every stage native; the result is the reference's `done` message
function handleGenerate(data) {
    const { N, P, jitter, nMag, numContinents, smoothing, hydraulicErosion, thermalErosion, ridgeSharpening, glacialErosion, terrainWarp,
            continentSizeVariety = 0, temperatureOffset = 0, precipitationOffset = 0, landCoverage = 0.3, seed: overrideSeed, toggledIndices } = data;
    if (!(Number.isInteger(N) && N >= 1 && Number.isInteger(P) && P >= 1)) {
        // the reference would throw inside buildSphere; the retained state, if any, is kept
        parentPort.postMessage({ type: 'error', message: 'generate needs N and P (a generate without them is not served by the device worker)' });
        return;
    }
    const timing = [];
    let replaced = false;
    try {
        const tTotal0 = performance.now();
        progress(0, 'Shaping the world…');
        const seed = (overrideSeed !== undefined && overrideSeed !== null) ? overrideSeed : Math.floor(Math.random() * 16777216);

        let t0 = performance.now();
        const built = buildSphere(N, jitter, seed, true, (data.deviceMesh || data.devicePoints) ? defaultContext() : null, !!data.devicePoints);       // deviceMesh: the device builder, the same arrays; devicePoints: the points from the device too
        const { mesh, r_xyz } = built;
        timing.push({ stage: 'Sphere mesh (Fibonacci + Delaunay + pole)', ms: performance.now() - t0 });
        t0 = performance.now();
        const neighborDist = built.neighborDist || computeNeighborDist(mesh, r_xyz);
        timing.push({ stage: 'Neighbor distances', ms: performance.now() - t0 });
        t0 = performance.now();
        const t_xyz = generateTriangleCenters(mesh, r_xyz);
        timing.push({ stage: 'Triangle centers', ms: performance.now() - t0 });

        progress(10, 'Generating coarse plates…');
        t0 = performance.now();
        const { coarseMesh, coarse_xyz, coarse_r_plate, coarsePlateSeeds, coarsePlateVec, coarsePlateIsOcean } =
            generateCoarsePlates(seed, P, numContinents, continentSizeVariety, landCoverage);
        timing.push({ stage: `Coarse plates (${P} plates, ${numContinents} continents)`, ms: performance.now() - t0 });

        progress(20, 'Projecting plates…');
        t0 = performance.now();
        releaseRetained();
        replaced = true;
        const planet = addon.planetCreate(defaultContext(), mesh.numRegions, mesh.adjOffset, mesh.adjList, r_xyz, neighborDist);
        W = { planet, numRegions: mesh.numRegions, triangles: mesh.triangles, halfedges: mesh.halfedges, seed, hasHotspot: false, r_plate: null, plateIsOcean: null,
              plateSeeds: null, plateVec: null, plateDensity: {}, P, cachedWind: null, cachedOcean: null, temperatureOffset, precipitationOffset, landCoverage };
        const r_plate = addon.projectCoarsePlates(planet, coarseMesh.adjOffset, coarseMesh.adjList, coarse_xyz, coarse_r_plate, seed, P);
        timing.push({ stage: 'Project coarse → hi-res', ms: performance.now() - t0 });

        progress(25, 'Smoothing boundaries…');
        t0 = performance.now();
        const seedArr = Int32Array.from(coarsePlateSeeds);
        addon.smoothAndReconnectPlates(mesh.numRegions, mesh.adjOffset, mesh.adjList, r_plate, seedArr, 3);
        timing.push({ stage: 'Smooth projected plates', ms: performance.now() - t0 });

        const plateSeeds = coarsePlateSeeds, plateVec = coarsePlateVec, plateIsOcean = coarsePlateIsOcean;
        const originalPlateIsOcean = new Set(plateIsOcean);
        if (toggledIndices && toggledIndices.length > 0) {
            for (const i of toggledIndices) {
                if (i < seedArr.length) {
                    const r = seedArr[i];
                    if (plateIsOcean.has(r)) plateIsOcean.delete(r); else plateIsOcean.add(r);
                }
            }
        }
        const { plateDensity, plateDensityLand, plateDensityOcean } = plateDensities(plateSeeds, plateIsOcean);

        W.r_plate = new Int32Array(r_plate);             // copies: r_plate's buffer leaves with the message
        W.plateSeeds = seedArr; W.plateVec = plateVec; W.plateIsOcean = Int32Array.from(plateIsOcean);
        W.originalPlateIsOcean = Int32Array.from(originalPlateIsOcean);
        W.plateDensity = Object.assign({}, plateDensity);
        W.plateDensityLand = Object.assign({}, plateDensityLand); W.plateDensityOcean = Object.assign({}, plateDensityOcean);
        W.nMag = nMag;

        const c = elevationChain({ smoothing, glacialErosion, hydraulicErosion, thermalErosion, ridgeSharpening, terrainWarp }, nMag, (stage) => {
            if (stage === 'elevation') progress(35, 'Raising mountains…');
            else if (stage === 'erosion') progress(60, 'Eroding terrain…');
            else progress(75, 'Computing triangle elevations…');
        });
        W.debugLayers = c.debugLayers;                    // what exportMap's generic layers read; the message clones them
        W.hasHotspot = true;                             // the call's hotspot layer stays on the device for the reapplies that follow
        if (c.sup) timing.push({ stage: `Super plates (${c.sup.numSuperPlates} groups from ${P} plates)`, ms: c.tSuper });
        timing.push({ stage: 'Elevation (collisions + stress + distance fields + assignment)', ms: c.tElev });
        timing.push({ stage: 'Terrain post-processing (total)', ms: c.tPost });
        timing.push({ stage: 'Triangle elevations', ms: c.tTriElev });
        timing.push({ stage: 'Clone state for retention', ms: 0 });          // the state is on the device already

        const climate = {};
        for (const k of CLIMATE_NULLS) climate[k] = null;
        const result = {
            type: 'done', triangles: mesh.triangles, halfedges: mesh.halfedges, numRegions: mesh.numRegions, r_xyz, t_xyz, r_plate,
            plateSeeds: Array.from(plateSeeds), plateVec, plateIsOcean: Array.from(plateIsOcean), originalPlateIsOcean: Array.from(originalPlateIsOcean),
            plateDensity, plateDensityLand, plateDensityOcean, prePostElev: c.prePostElev, r_elevation: c.r_elevation, t_elevation: c.t_elevation,
            mountain_r: Array.from(c.res.mountain), coastline_r: Array.from(c.res.coastline), ocean_r: Array.from(c.res.ocean), r_stress: c.res.r_stress,
            ...climate, skipClimate: true, seed, nMag, debugLayers: c.debugLayers,
            _timing: c._timing, _pipelineTiming: timing, _postTiming: c.postTiming, _workerTotal: performance.now() - tTotal0,
            _params: { N, P, jitter, nMag, numContinents, smoothing, terrainWarp, hydraulicErosion, thermalErosion, ridgeSharpening, glacialErosion,
                       continentSizeVariety, temperatureOffset, precipitationOffset, landCoverage, seed }
        };
        parentPort.postMessage(result, [r_xyz.buffer, t_xyz.buffer, r_plate.buffer, c.prePostElev.buffer, c.r_elevation.buffer, c.t_elevation.buffer, c.res.r_stress.buffer]);
    } catch (err) {
        if (replaced) releaseRetained();                 // the half-built state is no state: a following reapply answers `No retained state`
        parentPort.postMessage({ type: 'error', message: err.message, stack: err.stack });
    }
}

// js/planet-worker.js:104-110
function getClimateParams(data) {
    const pick = (k, dflt) => (data && data[k] !== undefined && data[k] !== null) ? data[k] : (W && W[k] !== undefined && W[k] !== null) ? W[k] : dflt;
    const temperatureOffset = pick('temperatureOffset', 0), precipitationOffset = pick('precipitationOffset', 0), landCoverage = pick('landCoverage', 0.3);
    if (W) { W.temperatureOffset = temperatureOffset; W.precipitationOffset = precipitationOffset; W.landCoverage = landCoverage; }
    return { temperatureOffset, precipitationOffset, landCoverage };
}

// js/planet-worker.js:579-677 with every stage on the device; the planet's resident elevation is r_elevation_final
function handleComputeClimate(data) {
    if (!W) { parentPort.postMessage({ type: 'error', message: 'No retained state for computeClimate' }); return; }
    if (!W.r_plate || !W.plateIsOcean) {
        const missing = [!W.r_plate ? 'r_plate' : null, !W.plateIsOcean ? 'plateIsOcean' : null].filter((k) => k).join(' and ');
        parentPort.postMessage({ type: 'error', message: `computeClimate: the retained state has no ${missing} (pass them to retain, or run importHeightmap)` });
        return;
    }
    const { temperatureOffset, precipitationOffset, landCoverage } = getClimateParams(data);
    try {
        const tTotal0 = performance.now();
        const planet = W.planet;
        let windResult = W.cachedWind, oceanResult = W.cachedOcean;
        let tWind = 0, tOcean = 0, t0;
        if (!windResult) {
            progress(0, 'Simulating wind patterns\u2026');
            t0 = performance.now();
            windResult = addon.computeWind(planet, null, W.r_plate, W.plateIsOcean, W.seed, 23.5);
            tWind = performance.now() - t0;

            progress(30, 'Computing ocean currents\u2026');
            t0 = performance.now();
            addon.computeOceanCurrents(planet);
            oceanResult = downloadAll(planet, addon.oceanDownload, OCEAN_KEYS);
            tOcean = performance.now() - t0;

            W.cachedWind = windResult;
            W.cachedOcean = oceanResult;
        }

        progress(50, 'Computing precipitation\u2026');
        t0 = performance.now();
        addon.computePrecipitation(planet, null, Number(precipitationOffset), Number(landCoverage));
        const precipResult = downloadAll(planet, addon.precipDownload, PRECIP_KEYS);
        const tPrecip = performance.now() - t0;

        progress(70, 'Computing temperature\u2026');
        t0 = performance.now();
        addon.computeTemperature(planet, null, Number(temperatureOffset));
        const tempResult = downloadAll(planet, addon.temperatureDownload, TEMP_KEYS);
        const tTemp = performance.now() - t0;

        progress(88, 'Classifying climates\u2026');
        t0 = performance.now();
        const koppen = addon.classifyKoppen(planet, null);
        const tKoppen = performance.now() - t0;

        const tWorkerTotal = performance.now() - tTotal0;
        const climateDebugLayers = {
            pressureSummer: windResult.r_pressure_summer, pressureWinter: windResult.r_pressure_winter,
            windSpeedSummer: windResult.r_wind_speed_summer, windSpeedWinter: windResult.r_wind_speed_winter,
            continentality: windResult.r_continentality,
            precipSummer: precipResult.r_precip_summer, precipWinter: precipResult.r_precip_winter,
            rainShadowSummer: precipResult.r_rainshadow_summer, rainShadowWinter: precipResult.r_rainshadow_winter,
            tempSummer: tempResult.r_temperature_summer, tempWinter: tempResult.r_temperature_winter,
            koppen
        };
        progress(95, 'Done');
        const climate = {};
        for (const k of CLIMATE_NULLS) climate[k] = k in windResult ? windResult[k] : k in oceanResult ? oceanResult[k] : k in precipResult ? precipResult[k] : tempResult[k];
        // no transfer list: the wind and ocean arrays stay in W for the next command, as the reference's cachedWind does
        parentPort.postMessage({ type: 'climateDone', ...climate, climateDebugLayers,
                                 _climateTiming: { wind: tWind, ocean: tOcean, precipitation: tPrecip, temperature: tTemp, koppen: tKoppen, workerTotal: tWorkerTotal } });
    } catch (err) {
        parentPort.postMessage({ type: 'error', message: err.message, stack: err.stack });
    }
}

// the types and layers an exportMap or exportCubeMap request asks for, checked
function requestedMaps(cmd, data) {
    const types = data.types !== undefined && data.types !== null ? Array.from(data.types) : [data.type];
    for (const t of types) if (MAP_TYPES.indexOf(t) < 0) throw new RangeError(`${cmd}: unknown map type '${t}' (one of ${MAP_TYPES.join(', ')})`);
    if (types.length === 0) throw new RangeError(`${cmd}: no map type given`);
    // a layer is a climate layer of the map view, read from the planet's resident block, or a key of the retained debugLayers
    const generic = W.debugLayers || {};
    const layers = (data.layers !== undefined && data.layers !== null ? Array.from(data.layers) : []).map((name) => {
        const id = MAP_LAYERS.indexOf(name);
        if (id > 0) return { name, id, values: null };
        if (name !== 'debug' && generic[name] instanceof Float32Array) return { name, id: 0, values: generic[name] };
        throw new RangeError(`${cmd}: unknown map layer '${name}' (one of ${MAP_LAYERS.slice(1).concat(Object.keys(generic)).join(', ')})`);
    });
    return { types, layers };
}

// js/planet-mesh.js:1965-2180 without the page: one raster, one colour pass per type, on W.planet's current elevation and Koppen block
function handleExportMap(data) {
    if (!W) { parentPort.postMessage({ type: 'error', message: 'No retained state for exportMap' }); return; }
    const missing = ['triangles', 'halfedges'].filter((k) => !(W[k] instanceof Int32Array));
    if (missing.length) {
        parentPort.postMessage({ type: 'error', message: `exportMap: the retained state has no mesh.${missing.join(' and mesh.')} (pass them to retain, or run importHeightmap)` });
        return;
    }
    try {
        const tTotal0 = performance.now();
        const { types, layers } = requestedMaps('exportMap', data);
        const width = data.width;
        const rivers = data.rivers !== undefined && data.rivers !== null ? checkedMinFlow('exportMap', data.rivers) : null;
        progress(0, 'Rendering...');
        let t0 = performance.now();
        const r = rasterOnPlanet(W.planet, W.triangles, W.halfedges, width, data.centerLon);
        const tRaster = performance.now() - t0;
        t0 = performance.now();
        const maps = [], total = types.length + layers.length;
        types.forEach((type, k) => {
            maps.push({ type, filename: exportFilename(type, W.seed), rgba: rivers === null ? addon.mapColor(W.planet, MAP_TYPES.indexOf(type), null, width)
                                                                                                 : addon.mapColorRivers(W.planet, MAP_TYPES.indexOf(type), null, rivers, width) });
            progress(80 * (k + 1) / total, 'Rendering...');
        });
        layers.forEach((l, k) => {
            maps.push({ type: l.name, filename: layerFilename(l.name, W.seed), rgba: addon.mapColorLayer(W.planet, l.id, l.values, null, width) });
            progress(80 * (types.length + k + 1) / total, 'Rendering...');
        });
        const tColor = performance.now() - t0;
        let tEncode = 0;
        if (data.png) {
            progress(85, 'Encoding PNG...');
            t0 = performance.now();
            for (const m of maps) m.png = encodePng(m.rgba, r.width, r.height);
            tEncode = performance.now() - t0;
        }
        const transfer = [];
        for (const m of maps) { transfer.push(m.rgba.buffer); if (m.png) transfer.push(m.png.buffer); }
        parentPort.postMessage({ type: 'exportDone', width: r.width, height: r.height, maps,
                                 _exportTiming: { raster: tRaster, color: tColor, encode: tEncode, workerTotal: performance.now() - tTotal0 } }, transfer);
    } catch (err) {
        parentPort.postMessage({ type: 'error', message: err.message, stack: err.stack });
    }
}

// ours: the relief of W.planet's current elevation on the map or on the cube: one relief raster, one pass per kind
function handleExportRelief(data) {
    if (!W) { parentPort.postMessage({ type: 'error', message: 'No retained state for exportRelief' }); return; }
    const missing = ['triangles', 'halfedges'].filter((k) => !(W[k] instanceof Int32Array));
    if (missing.length) {
        parentPort.postMessage({ type: 'error', message: `exportRelief: the retained state has no mesh.${missing.join(' and mesh.')} (pass them to retain, or run importHeightmap)` });
        return;
    }
    try {
        const tTotal0 = performance.now();
        const kinds = data.kinds !== undefined && data.kinds !== null ? Array.from(data.kinds) : [];
        if (kinds.length === 0) throw new RangeError(`exportRelief: no relief kind given (some of ${RELIEF_KINDS.join(', ')})`);
        const projection = data.projection === undefined || data.projection === null ? 'map' : data.projection;
        if (projection !== 'map' && projection !== 'cube') throw new RangeError(`exportRelief: unknown projection '${projection}' (one of map, cube)`);
        const layout = data.layout === undefined || data.layout === null ? 'faces' : data.layout;
        if (layout !== 'faces' && layout !== 'column') throw new RangeError(`exportRelief: unknown layout '${layout}' (one of faces, column)`);
        const opts = { centerLon: data.centerLon, strength: data.strength, flatOcean: !!data.flatOcean };
        const encode = (m, w, h) => (reliefIs16(m.kind) ? encodePng16(m.data, w, h) : encodePng(m.data, w, h));
        progress(0, 'Rendering...');
        let t0 = performance.now(), tEncode = 0;
        if (projection === 'map') {
            const width = data.width;
            if (!(Number.isInteger(width) && width >= 2 && width <= 32768 && width % 2 === 0)) throw new RangeError('exportRelief: width must be an even integer from 2 to 32768');
            const r = exportReliefOnPlanet(W.planet, W.triangles, W.halfedges, null, kinds, width, opts);
            const tRender = performance.now() - t0;
            const maps = r.maps.map((m) => ({ kind: m.kind, filename: reliefFilename(m.kind, W.seed), data: m.data }));
            if (data.png) {
                progress(85, 'Encoding PNG...');
                t0 = performance.now();
                for (const m of maps) m.png = encode(m, r.width, r.height);
                tEncode = performance.now() - t0;
            }
            const transfer = [];
            for (const m of maps) { transfer.push(m.data.buffer); if (m.png) transfer.push(m.png.buffer); }
            parentPort.postMessage({ type: 'exportReliefDone', projection, width: r.width, height: r.height, covered: r.covered, uncovered: r.uncovered, maps,
                                     _exportTiming: { render: tRender, encode: tEncode, workerTotal: performance.now() - tTotal0 } }, transfer);
            return;
        }
        const S = data.faceSize;
        if (!(Number.isInteger(S) && S >= 1 && S <= CUBE_MAX_FACE_SIZE)) throw new RangeError('exportRelief: faceSize must be an integer from 1 to 16384');
        const r = exportCubeReliefOnPlanet(W.planet, W.triangles, W.halfedges, null, kinds, S, opts);
        const tRender = performance.now() - t0;
        const maps = r.maps.map((m) => ({                                      // one S x 6S image per kind; the faces are views of it
            kind: m.kind,
            faces: layout === 'column' ? [{ face: 'column', filename: reliefFilename(m.kind, W.seed, 'column'), kind: m.kind, data: m.data }]
                : reliefFaces(m.data, S, reliefIs16(m.kind) ? 1 : 4).map((f) => ({ face: f.face, filename: reliefFilename(m.kind, W.seed, f.face), kind: m.kind, data: f.data }))
        }));
        if (data.png) {
            progress(85, 'Encoding PNG...');
            t0 = performance.now();
            for (const m of maps) for (const f of m.faces) f.png = encode(f, S, layout === 'column' ? 6 * S : S);
            tEncode = performance.now() - t0;
        }
        const transfer = r.maps.map((m) => m.data.buffer);                     // each image's one buffer; the six views travel with it
        for (const m of maps) for (const f of m.faces) if (f.png) transfer.push(f.png.buffer);
        parentPort.postMessage({ type: 'exportReliefDone', projection, faceSize: S, covered: r.covered, uncovered: r.uncovered, maps,
                                 _exportTiming: { render: tRender, encode: tEncode, workerTotal: performance.now() - tTotal0 } }, transfer);
    } catch (err) {
        parentPort.postMessage({ type: 'error', message: err.message, stack: err.stack });
    }
}

// ours: the globe of W.planet's current elevation and Koppen block through a camera: one view raster, one colour pass per type and layer
function handleRenderGlobe(data) {
    if (!W) { parentPort.postMessage({ type: 'error', message: 'No retained state for renderGlobe' }); return; }
    const missing = ['triangles', 'halfedges'].filter((k) => !(W[k] instanceof Int32Array));
    if (missing.length) {
        parentPort.postMessage({ type: 'error', message: `renderGlobe: the retained state has no mesh.${missing.join(' and mesh.')} (pass them to retain, or run importHeightmap)` });
        return;
    }
    try {
        const tTotal0 = performance.now();
        const { types, layers } = requestedMaps('renderGlobe', data);
        const width = data.width, height = data.height;
        for (const [k, v] of [['width', width], ['height', height]])
            if (!(Number.isInteger(v) && v >= 1 && v <= VIEW_MAX_SIZE)) throw new RangeError(`renderGlobe: ${k} must be an integer from 1 to 16384`);
        const rivers = data.rivers !== undefined && data.rivers !== null ? checkedMinFlow('renderGlobe', data.rivers) : null;
        const params = viewParams(data);
        progress(0, 'Rendering...');
        let t0 = performance.now();
        const r = addon.viewRaster(W.planet, W.triangles, W.halfedges, width, height, params, null, false);
        const tRaster = performance.now() - t0;
        t0 = performance.now();
        const maps = [], total = types.length + layers.length;
        types.forEach((type, k) => {
            maps.push({ type, filename: viewFilename(type, W.seed), rgba: rivers === null ? addon.mapColor(W.planet, MAP_TYPES.indexOf(type), null)
                                                                                               : addon.mapColorRivers(W.planet, MAP_TYPES.indexOf(type), null, rivers) });
            progress(80 * (k + 1) / total, 'Rendering...');
        });
        layers.forEach((l, k) => {
            maps.push({ type: l.name, filename: viewFilename(l.name, W.seed), rgba: addon.mapColorLayer(W.planet, l.id, l.values, null) });
            progress(80 * (types.length + k + 1) / total, 'Rendering...');
        });
        const tColor = performance.now() - t0;
        let tEncode = 0;
        if (data.png) {
            progress(85, 'Encoding PNG...');
            t0 = performance.now();
            for (const m of maps) m.png = encodePng(m.rgba, r.width, r.height);
            tEncode = performance.now() - t0;
        }
        const transfer = [];
        for (const m of maps) { transfer.push(m.rgba.buffer); if (m.png) transfer.push(m.png.buffer); }
        parentPort.postMessage({ type: 'renderGlobeDone', width: r.width, height: r.height, covered: r.covered, uncovered: r.uncovered, maps,
                                 _exportTiming: { raster: tRaster, color: tColor, encode: tEncode, workerTotal: performance.now() - tTotal0 } }, transfer);
    } catch (err) {
        parentPort.postMessage({ type: 'error', message: err.message, stack: err.stack });
    }
}

// ours: the cube map of W.planet's current elevation and Koppen block: one raster of the six faces, one colour pass per type and layer
function handleExportCubeMap(data) {
    if (!W) { parentPort.postMessage({ type: 'error', message: 'No retained state for exportCubeMap' }); return; }
    const missing = ['triangles', 'halfedges'].filter((k) => !(W[k] instanceof Int32Array));
    if (missing.length) {
        parentPort.postMessage({ type: 'error', message: `exportCubeMap: the retained state has no mesh.${missing.join(' and mesh.')} (pass them to retain, or run importHeightmap)` });
        return;
    }
    try {
        const tTotal0 = performance.now();
        const { types, layers } = requestedMaps('exportCubeMap', data);
        const S = data.faceSize, layout = data.layout === undefined || data.layout === null ? 'faces' : data.layout;
        if (!(Number.isInteger(S) && S >= 1 && S <= CUBE_MAX_FACE_SIZE)) throw new RangeError('exportCubeMap: faceSize must be an integer from 1 to 16384');
        if (layout !== 'faces' && layout !== 'column') throw new RangeError(`exportCubeMap: unknown layout '${layout}' (one of faces, column)`);
        const rivers = data.rivers !== undefined && data.rivers !== null ? checkedMinFlow('exportCubeMap', data.rivers) : null;
        progress(0, 'Rendering...');
        let t0 = performance.now();
        addon.mapRasterCube(W.planet, W.triangles, W.halfedges, S, false);
        const tRaster = performance.now() - t0;
        t0 = performance.now();
        const images = [], total = types.length + layers.length;             // one S x 6S image per map; the faces are views of it
        types.forEach((type, k) => {
            images.push({ type, rgba: rivers === null ? addon.mapColor(W.planet, MAP_TYPES.indexOf(type), null) : addon.mapColorRivers(W.planet, MAP_TYPES.indexOf(type), null, rivers) });
            progress(80 * (k + 1) / total, 'Rendering...');
        });
        layers.forEach((l, k) => {
            images.push({ type: l.name, rgba: addon.mapColorLayer(W.planet, l.id, l.values, null) });
            progress(80 * (types.length + k + 1) / total, 'Rendering...');
        });
        const tColor = performance.now() - t0;
        const stem = (type) => cubeFilename(type, 'px', W.seed).slice(0, -'-px.png'.length);
        const maps = images.map((m) => ({
            type: m.type,
            faces: layout === 'column' ? [{ face: 'column', filename: `${stem(m.type)}-column.png`, rgba: m.rgba }]
                : cubeFaces(m.rgba, S).map((f) => ({ face: f.face, filename: cubeFilename(m.type, f.face, W.seed), rgba: f.rgba }))
        }));
        let tEncode = 0;
        if (data.png) {
            progress(85, 'Encoding PNG...');
            t0 = performance.now();
            for (const m of maps) for (const f of m.faces) f.png = encodePng(f.rgba, S, layout === 'column' ? 6 * S : S);
            tEncode = performance.now() - t0;
        }
        const transfer = images.map((m) => m.rgba.buffer);                     // each image's one buffer; the six views travel with it
        for (const m of maps) for (const f of m.faces) if (f.png) transfer.push(f.png.buffer);
        parentPort.postMessage({ type: 'exportCubeDone', faceSize: S, maps,
                                 _exportTiming: { raster: tRaster, color: tColor, encode: tEncode, workerTotal: performance.now() - tTotal0 } }, transfer);
    } catch (err) {
        parentPort.postMessage({ type: 'error', message: err.message, stack: err.stack });
    }
}

// what the overlay requests of exportGlobe and exportOverlays share
function checkedSeason(cmd, key, season) {
    if (SEASONS.indexOf(season) < 0) throw new RangeError(`${cmd}: ${key} takes a season ('summer' or 'winter'), not '${season}'`);
    return season;
}
function itczOf(cmd, season) {
    checkedSeason(cmd, 'itcz', season);
    const wind = W.cachedWind;
    if (!wind || !(wind.itczLons instanceof Float32Array)) throw new Error(`${cmd}: no wind result on this planet (run computeClimate first)`);
    return { itczLons: wind.itczLons, itczLats: season === 'winter' ? wind.itczLatsWinter : wind.itczLatsSummer };
}

// js/planet-mesh.js:1289-1749, :385-469 without the page: the arrows, the ITCZ line and the grids, each in the globe and the map form
function handleExportOverlays(data) {
    if (!W) { parentPort.postMessage({ type: 'error', message: 'No retained state for exportOverlays' }); return; }
    try {
        const tTotal0 = performance.now();
        const centerLon = Number(data.centerLon) || 0;
        const msg = { type: 'overlaysDone', centerLon }, transfer = [];
        const asked = (k) => data[k] !== undefined && data[k] !== null;
        if (asked('windArrows')) msg.windArrows = windArrowsOnPlanet(W.planet, checkedSeason('exportOverlays', 'windArrows', data.windArrows), centerLon);
        if (asked('oceanCurrentArrows')) msg.oceanCurrentArrows = oceanCurrentArrowsOnPlanet(W.planet, checkedSeason('exportOverlays', 'oceanCurrentArrows', data.oceanCurrentArrows), centerLon, null);
        if (asked('itcz')) { const src = itczOf('exportOverlays', data.itcz); msg.itcz = itczLine(src.itczLons, src.itczLats); }
        if (asked('grid')) msg.grid = grids(data.grid, centerLon);
        for (const k of ['windArrows', 'oceanCurrentArrows']) if (msg[k]) transfer.push(msg[k].globe.position.buffer, msg[k].globe.color.buffer, msg[k].map.position.buffer, msg[k].map.color.buffer);
        for (const k of ['itcz', 'grid']) if (msg[k]) transfer.push(msg[k].globe.buffer, msg[k].map.buffer);
        msg._overlayTiming = { workerTotal: performance.now() - tTotal0 };
        parentPort.postMessage(msg, transfer);
    } catch (err) {
        parentPort.postMessage({ type: 'error', message: err.message, stack: err.stack });
    }
}

// js/planet-mesh.js:620-836 without the page: the globe mesh of W.planet's current elevation in one view, its line sets, and the GLB file
function handleExportGlobe(data) {
    if (!W) { parentPort.postMessage({ type: 'error', message: 'No retained state for exportGlobe' }); return; }
    const missing = ['triangles', 'halfedges'].filter((k) => !(W[k] instanceof Int32Array));
    if (missing.length) {
        parentPort.postMessage({ type: 'error', message: `exportGlobe: the retained state has no mesh.${missing.join(' and mesh.')} (pass them to retain, or run importHeightmap)` });
        return;
    }
    try {
        const tTotal0 = performance.now();
        const generic = W.debugLayers || {};
        let view = 'color';
        const opts = { wireframe: !!data.wireframe, glb: !!data.glb };
        if (data.plates) {
            const seeds = W.plateSeeds || W.syntheticSeeds;
            if (!W.r_plate || !seeds || !W.plateIsOcean) throw new Error('exportGlobe: the plate view needs r_plate, plateSeeds and plateIsOcean in the retained state');
            view = GLOBE_PLATES;
            opts.plates = { r_plate: W.r_plate, plateSeeds: seeds, plateColors: computePlateColors(seeds, W.plateIsOcean) };
        } else if (data.layer !== undefined && data.layer !== null) {
            const name = data.layer;
            if (MAP_LAYERS.indexOf(name) > 0) view = name;
            else if (name !== 'debug' && generic[name] instanceof Float32Array) { view = 'debug'; opts.values = generic[name]; }
            else throw new RangeError(`exportGlobe: unknown map layer '${name}' (one of ${MAP_LAYERS.slice(1).concat(Object.keys(generic)).join(', ')})`);
        } else if (data.view !== undefined && data.view !== null) {
            if (GLOBE_TYPE_VIEWS.indexOf(data.view) < 0) throw new RangeError(`exportGlobe: unknown globe view '${data.view}' (one of ${GLOBE_TYPE_VIEWS.join(', ')})`);
            view = data.view;
        }
        if (data.superPlateBorders instanceof Float32Array) opts.superPlates = data.superPlateBorders;      // the caller's own field
        else if (data.superPlateBorders) {
            if (!(generic.superPlates instanceof Float32Array)) throw new Error('exportGlobe: the retained debugLayers have no superPlates (generate or editRecompute with P >= 8 leaves them)');
            opts.superPlates = generic.superPlates;
        }
        for (const k of ['windArrows', 'oceanCurrentArrows']) if (data[k] !== undefined && data[k] !== null) opts[k] = checkedSeason('exportGlobe', k, data[k]);
        if (data.itcz !== undefined && data.itcz !== null) opts.itcz = itczOf('exportGlobe', data.itcz);
        if (data.grid !== undefined && data.grid !== null) opts.grid = data.grid;
        if (data.rivers !== undefined && data.rivers !== null) opts.rivers = { minFlow: checkedMinFlow('exportGlobe', data.rivers) };
        if (data.outlines !== undefined && data.outlines !== null) {
            const req = outlineRequest('exportGlobe', data.outlines);
            opts.outlines = Object.assign({}, req.opts, { source: req.source });
        }
        progress(0, 'Building globe...');
        const name = data.plates ? GLOBE_PLATES : (data.layer !== undefined && data.layer !== null ? data.layer : view);
        const res = exportGlobeOnPlanet(W.planet, W.triangles, W.halfedges, null, view, W.seed, opts);
        progress(90, 'Done');
        const msg = { type: 'globeDone', view: name, filename: globeFilename(name, W.seed), numSides: W.triangles.length, bounds: res.bounds };
        const transfer = [];
        if (res.glb) { msg.glb = res.glb; transfer.push(res.glb.buffer); }
        else {
            msg.position = res.position; msg.color = res.color;
            transfer.push(res.position.buffer, res.color.buffer);
            for (const k of ['wireframe', 'superPlateBorders', 'itcz', 'grid', 'rivers', 'outlines']) if (res[k]) { msg[k] = res[k]; transfer.push(res[k].buffer); }
            for (const k of ['windArrows', 'oceanCurrentArrows']) if (res[k]) { msg[k] = res[k]; transfer.push(res[k].position.buffer, res[k].color.buffer); }
        }
        msg._globeTiming = { workerTotal: performance.now() - tTotal0 };
        parentPort.postMessage(msg, transfer);
    } catch (err) {
        parentPort.postMessage({ type: 'error', message: err.message, stack: err.stack });
    }
}

// a command's { source, levels, values, onlyClass } -> what buildOutlineOnPlanet takes; 'plates' and 'superPlates' pass the worker's own arrays as values
function outlineRequest(fn, data) {
    if (!data || typeof data !== 'object' || typeof data.source !== 'string') throw new TypeError(`${fn}: outlines take { source, levels?, values?, onlyClass? }`);
    const req = { name: data.source, source: data.source, opts: { levels: data.levels, values: data.values, onlyClass: data.onlyClass } };
    if (data.source === 'plates') {
        if (!(W.r_plate instanceof Int32Array)) throw new Error(`${fn}: the retained state has no r_plate`);
        req.source = 'values'; req.opts.values = W.r_plate;
    } else if (data.source === 'superPlates') {
        const sp = (W.debugLayers || {}).superPlates;
        if (!(sp instanceof Float32Array)) throw new Error(`${fn}: the retained debugLayers have no superPlates (generate or editRecompute with P >= 8 leaves them)`);
        // the borders compare floats, a NaN differs from everything: as int32 classes every NaN cell gets a class of its own
        req.source = 'values'; req.opts.values = Int32Array.from(sp, (v, r) => (Number.isNaN(v) ? -1 - r : v));
    } else if (OUTLINE_SOURCES.indexOf(data.source) < 0) {
        throw new RangeError(`${fn}: unknown outline source '${data.source}' (one of ${OUTLINE_SOURCES.concat(['plates', 'superPlates']).join(', ')})`);
    }
    return req;
}

// ours: the outlines of W.planet's current state as rings, as arrays or written out
function handleExportOutlines(data) {
    if (!W) { parentPort.postMessage({ type: 'error', message: 'No retained state for exportOutlines' }); return; }
    const missing = ['triangles', 'halfedges'].filter((k) => !(W[k] instanceof Int32Array));
    if (missing.length) {
        parentPort.postMessage({ type: 'error', message: `exportOutlines: the retained state has no mesh.${missing.join(' and mesh.')} (pass them to retain, or run importHeightmap)` });
        return;
    }
    try {
        const tTotal0 = performance.now();
        const format = data.format === undefined || data.format === null ? 'arrays' : data.format;
        if (['arrays', 'geojson', 'svg'].indexOf(format) < 0) throw new RangeError(`exportOutlines: unknown format '${format}' (one of arrays, geojson, svg)`);
        const req = outlineRequest('exportOutlines', data);
        progress(0, 'Tracing outlines...');
        const res = buildOutlineOnPlanet(W.planet, W.triangles, W.halfedges, req.source, Object.assign({}, req.opts, { lonlat: true }));
        progress(90, 'Done');
        const msg = { type: 'outlinesDone', source: req.name, format, ...res.info, filename: outlineFilename(req.name, W.seed, format === 'svg' ? 'svg' : 'geojson') };
        const transfer = [];
        if (format === 'arrays') {
            for (const k of OUTLINE_FIELDS.concat(['lonlat'])) { msg[k] = res[k]; transfer.push(res[k].buffer); }
        } else if (format === 'geojson') msg.text = outlineToGeoJSON(res, { source: req.name });
        else msg.text = outlineToSvg(res, data.width === undefined || data.width === null ? 2048 : data.width, data.centerLon || 0);
        msg._outlineTiming = { workerTotal: performance.now() - tTotal0 };
        parentPort.postMessage(msg, transfer);
    } catch (err) {
        parentPort.postMessage({ type: 'error', message: err.message, stack: err.stack });
    }
}

// ours: the rivers and lakes of W.planet's current elevation, resident for the exports
function handleComputeRivers(data) {
    if (!W) { parentPort.postMessage({ type: 'error', message: 'No retained state for computeRivers' }); return; }
    try {
        const tTotal0 = performance.now();
        progress(0, 'Tracing rivers...');
        const res = computeRiversOnPlanet(W.planet, null, data.runoff, !!data.download);
        progress(90, 'Done');
        const transfer = [];
        for (const k of RIVER_KEYS) if (res[k]) transfer.push(res[k].buffer);
        parentPort.postMessage({ type: 'riversDone', ...res, _riversTiming: { workerTotal: performance.now() - tTotal0 } }, transfer);
    } catch (err) {
        parentPort.postMessage({ type: 'error', message: err.message, stack: err.stack });
    }
}

// js/edit-mode.js:18-93 without the page: the regions and plates under a batch of pointers
function handlePick(data) {
    if (!W) { parentPort.postMessage({ type: 'error', message: 'No retained state for pick' }); return; }
    try {
        const given = ['directions', 'rays', 'map'].filter((k) => data[k] !== undefined && data[k] !== null);
        if (given.length !== 1) throw new TypeError('pick: exactly one of directions, rays and map: { points, centerLon } is expected');
        let directions;
        if (data.directions) {
            if (data.directions.length % 3) throw new RangeError('pick: directions must hold three numbers per query');
            directions = Float64Array.from(data.directions);
        } else if (data.rays) directions = hitDirectionsGlobe(data.rays).directions;
        else {
            if (!data.map.points) throw new TypeError('pick: map takes { points, centerLon }');
            directions = hitDirectionsMap(data.map.points, Number(data.map.centerLon) || 0).directions;
        }
        if (directions.length / 3 > PICK_MAX_QUERIES) throw new RangeError(`pick: ${directions.length / 3} queries in one call, at most ${PICK_MAX_QUERIES}`);
        const regions = findNearestRegions(W.planet, directions).regions;
        const plates = new Int32Array(regions.length).fill(-1);
        if (W.r_plate) for (let i = 0; i < regions.length; i++) if (regions[i] >= 0) plates[i] = W.r_plate[regions[i]];
        parentPort.postMessage({ type: 'picked', regions, plates }, [regions.buffer, plates.buffer]);
    } catch (err) {
        parentPort.postMessage({ type: 'error', message: err.message, stack: err.stack });
    }
}

// js/planet-mesh.js:953-1244 without the page: the editor state whose tints the exports show
function handleSetHighlight(data) {
    if (!W) { parentPort.postMessage({ type: 'error', message: 'No retained state for setHighlight' }); return; }
    try {
        const pending = Array.from(data.pendingToggles || []);
        const hoveredPlate = (data.hoveredPlate === undefined || data.hoveredPlate === null) ? -1 : Number(data.hoveredPlate);
        const hoveredKoppen = (data.hoveredKoppen === undefined || data.hoveredKoppen === null) ? -1 : Number(data.hoveredKoppen);
        if (pending.length === 0 && !(hoveredPlate >= 0) && !(hoveredKoppen >= 0)) {
            clearHighlight(W.planet);
            parentPort.postMessage({ type: 'highlightSet', cleared: true, counts: { pendingOcean: 0, pendingLand: 0, hoveredPlate: 0, hoveredKoppen: 0 } });
            return;
        }
        if (!W.r_plate) throw new Error('setHighlight: the retained state has no r_plate (pass it to retain, or run generate or importHeightmap)');
        if (pending.length && !W.plateIsOcean) throw new Error('setHighlight: the retained state has no plateIsOcean, which says how a pending plate is tinted');
        const counts = setHighlight(W.planet, W.r_plate, pending, W.plateIsOcean || [], hoveredPlate, hoveredKoppen);
        parentPort.postMessage({ type: 'highlightSet', cleared: false, counts });
    } catch (err) {
        parentPort.postMessage({ type: 'error', message: err.message, stack: err.stack });
    }
}

parentPort.on('message', (data) => {
    const { cmd } = data;
    switch (cmd) {
        case 'retain': handleRetain(data); break;
        case 'reapply': handleReapply(data); break;
        case 'importHeightmap': handleImportHeightmap(data); break;
        case 'dispose': releaseRetained(); parentPort.postMessage({ type: 'disposed' }); break;
        case 'computeClimate': handleComputeClimate(data); break;
        case 'editRecompute': handleEditRecompute(data); break;
        case 'exportMap': handleExportMap(data); break;
        case 'exportCubeMap': handleExportCubeMap(data); break;
        case 'exportRelief': handleExportRelief(data); break;
        case 'renderGlobe': handleRenderGlobe(data); break;
        case 'exportGlobe': handleExportGlobe(data); break;
        case 'computeRivers': handleComputeRivers(data); break;
        case 'exportOutlines': handleExportOutlines(data); break;
        case 'exportOverlays': handleExportOverlays(data); break;
        case 'generate': handleGenerate(data); break;
        case 'pick': handlePick(data); break;
        case 'setHighlight': handleSetHighlight(data); break;
        default: parentPort.postMessage({ type: 'error', message: `Unknown command: ${cmd}` });
    }
});
