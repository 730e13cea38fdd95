// The editor's hit test and highlights without the page (the reference's js/edit-mode.js:18-93 and the highlight functions of
// js/planet-mesh.js:953-1244), on a device-resident planet.  ES module, Node >= 12.
//
// findNearestRegion keeps the reference's name: the region with the greatest dot product, the lowest index among equals, found on
// the device for many directions at once (csrc/pick.hip).  hitDirectionGlobe / hitDirectionMap are the arithmetic of getHitInfoGlobe
// (:43-59) and getHitInfoMap (:77-92) as the reference writes it, with Math.*: on Node that is the reference's own arithmetic, and
// it equals the library's front ends (wo_pick_directions_globe / wo_pick_directions_map) word for word.  Three's camera and
// matrices are the caller's business: a ray comes in the planet's local space with a normalised direction, a map point as wx, wy on
// the map plane.  setHighlight / clearHighlight set and drop the editor state the exports then show.  There is no JavaScript fallback.
import addon from './native.js';

export const PICK_MAX_QUERIES = 65536;

// directions: Float64Array, three per query -> { regions: Int32Array (-1: none), dots: Float64Array (the winning dot, or -2) }
export function findNearestRegions(planet, directions) {
    if (!(directions instanceof Float64Array)) directions = Float64Array.from(directions);
    return addon.pickRegions(planet, directions);
}
// the reference's call: one direction -> { region, plate } or null
export function findNearestRegion(planet, r_plate, nx, ny, nz) {
    const region = addon.pickRegions(planet, Float64Array.of(nx, ny, nz)).regions[0];
    if (region < 0) return null;
    return { region, plate: r_plate ? r_plate[region] : -1 };
}

// getHitInfoGlobe's arithmetic: the unit direction of the hit point, or null where the ray misses the sphere of radius 1.08
export function hitDirectionGlobe(ox, oy, oz, dx, dy, dz) {
    const R = 1.08;
    const b = 2 * (ox * dx + oy * dy + oz * dz);
    const c = ox * ox + oy * oy + oz * oz - R * R;
    const disc = b * b - 4 * c;
    if (disc < 0) return null;
    const t = (-b - Math.sqrt(disc)) * 0.5;
    if (t < 0) return null;
    const hx = ox + t * dx, hy = oy + t * dy, hz = oz + t * dz;
    const len = Math.sqrt(hx * hx + hy * hy + hz * hz) || 1;
    return [hx / len, hy / len, hz / len];
}
// getHitInfoMap's arithmetic: the direction under the map point (wx, wy), or null outside the map
export function hitDirectionMap(wx, wy, mapCenterLon) {
    const PI = Math.PI;
    const sx = 2 / PI;
    let lon = wx / sx + (mapCenterLon || 0);
    const lat = wy / sx;
    if (lat < -PI / 2 || lat > PI / 2) return null;
    if (lon > PI) lon -= 2 * PI;
    else if (lon < -PI) lon += 2 * PI;
    const cosLat = Math.cos(lat);
    return [cosLat * Math.sin(lon), Math.sin(lat), cosLat * Math.cos(lon)];
}
function directionsOf(count, at) {
    const directions = new Float64Array(3 * count).fill(NaN), valid = new Uint8Array(count);
    for (let i = 0; i < count; i++) {
        const d = at(i);
        if (d) { directions.set(d, 3 * i); valid[i] = 1; }
    }
    return { directions, valid };
}
// rays: six doubles per query (origin, direction) -> { directions: Float64Array (NaN where there is no hit), valid: Uint8Array }
export function hitDirectionsGlobe(rays) {
    if (rays.length % 6) throw new RangeError('hitDirectionsGlobe: rays must hold six numbers per query');
    return directionsOf(rays.length / 6, (i) => hitDirectionGlobe(rays[6 * i], rays[6 * i + 1], rays[6 * i + 2], rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]));
}
// points: wx, wy per query -> as hitDirectionsGlobe
export function hitDirectionsMap(points, mapCenterLon) {
    if (points.length % 2) throw new RangeError('hitDirectionsMap: points must hold two numbers per query');
    return directionsOf(points.length / 2, (i) => hitDirectionMap(points[2 * i], points[2 * i + 1], mapCenterLon));
}

// the editor state: pendingToggles (plate ids queued for a rebuild), plateIsOcean (the plates that are ocean now), hoveredPlate and
// hoveredKoppen as the reference's state holds them (-1: none) -> { pendingOcean, pendingLand, hoveredPlate, hoveredKoppen }, the
// regions per tint.  While it is set, globeMesh / globeMeshPlates / mapColor / mapColorLayer give the tinted colours.
export function setHighlight(planet, r_plate, pendingToggles, plateIsOcean, hoveredPlate = -1, hoveredKoppen = -1) {
    const ocean = new Set(plateIsOcean || []);
    const pending = Int32Array.from(pendingToggles || []);
    const isOcean = Uint8Array.from(pending, (id) => (ocean.has(id) ? 1 : 0));
    return addon.highlightSet(planet, r_plate, pending, isOcean, hoveredPlate, hoveredKoppen);
}
export function clearHighlight(planet) { addon.highlightClear(planet); }
