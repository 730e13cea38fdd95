// Counterpart of the reference's line overlays (js/planet-mesh.js) for hosts without WebGL: the wind and ocean-current arrows
// (buildWindArrows :1289-1465, buildOceanCurrentArrows :1545-1720) from HIP kernels (csrc/overlay.hip) on the planet bound to `mesh`
// (native.js: planetFor), and on the host the ITCZ line of the pressure views (:1498-1538) and the latitude / longitude grids
// (buildGlobeGrid :427-469, buildMapGrid :385-412).  Every array is the Float32Array the reference hands to three.js, bit for bit;
// planet_heightmap_generation_amd/overlay_export.py states the same functions and gives the same bytes.  Each overlay comes in the
// globe form and the map form.  The map form of the ITCZ line does not subtract the centre meridian: the reference's behaviour, kept.
// There is no JavaScript fallback for the arrows.
import addon, { planetFor } from './native.js';

export const OVERLAY_BINS = 7200;                           // 60 x 120 cells of 3 x 3 degrees
export const SEASONS = ['summer', 'winter'];
export { ARROW_OPACITY, ITCZ_COLOR, GRID_OPACITY } from './globe-glb.js';
export { itczLine, globeGrid, mapGrid, grids } from './overlay-lines.js';

function seasonId(season, fn) {
    const s = SEASONS.indexOf(season);
    if (s < 0) throw new RangeError(`${fn}: unknown season '${season}' (one of ${SEASONS.join(', ')})`);
    return s;
}

// ---- the device calls --------------------------------------------------------------------------------------------------------
// on a planet handle (what the worker holds); r_elevation null: the planet's resident field
export function gridRegionsOnPlanet(planet, skipLand, r_elevation) { return addon.overlayBins(planet, !!skipLand, skipLand ? (r_elevation || null) : null); }
export function windArrowsOnPlanet(planet, season, centerLon) { return addon.overlayArrows(planet, 0, seasonId(season, 'buildWindArrows'), Number(centerLon) || 0, null); }
export function oceanCurrentArrowsOnPlanet(planet, season, centerLon, r_elevation) {
    return addon.overlayArrows(planet, 1, seasonId(season, 'buildOceanCurrentArrows'), Number(centerLon) || 0, r_elevation || null);
}
// buildWindArrows(mesh, r_xyz, season, centerLon = 0) -> { globe: { position, color }, map: { position, color }, count }; the wind
// block is the planet's (computeWind, or windUpload of the season's r_wind_east_* and r_wind_north_*)
export function buildWindArrows(mesh, r_xyz, season, centerLon) { return windArrowsOnPlanet(planetFor(mesh, r_xyz), season, centerLon); }
// buildOceanCurrentArrows(mesh, r_xyz, r_elevation, season, centerLon = 0): land (r_elevation > 0) takes no part
export function buildOceanCurrentArrows(mesh, r_xyz, r_elevation, season, centerLon) { return oceanCurrentArrowsOnPlanet(planetFor(mesh, r_xyz), season, centerLon, r_elevation); }
