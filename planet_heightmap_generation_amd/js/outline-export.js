// Region outlines for hosts of the worker (ours: the reference exports no outline): the line where one class of cells ends and another
// begins (a coastline, a lake shore, a plate, a Koppen zone, an elevation band) traced into ordered closed rings.  Everything runs in
// HIP kernels (csrc/outline.hip; the contract is in csrc/outline_ops.h) on the planet bound to `mesh` (native.js: planetFor); there is
// no JavaScript fallback.  The rings stay on the planet until the next build.  The writers mirror outline_export.py: the same cuts,
// the same numbers.
import addon, { planetFor } from './native.js';

// the sources in the order of WO_OUTLINE_COAST, _LAKES, _KOPPEN, _LEVELS, _VALUES (include/worogen.h)
export const OUTLINE_SOURCES = ['coast', 'lakes', 'koppen', 'levels', 'values'];
export const OUTLINE_FIELDS = ['sides', 'ring_start', 'ring_class', 'ring_of_side'];
export const OUTLINE_GLOBE_BASE = 1.002;                    // where exportGlobe draws the rings: the base of the super-plate borders

// the file name of an outline export.  Ours: the reference exports no outline.
export function outlineFilename(source, seed, ext) { return `orogen-outline-${source}-${seed}.${ext || 'geojson'}`; }

// on a planet handle (what the worker holds).  opts: { r_elevation, values: Int32Array, levels, onlyClass, base, lonlat }; r_elevation
// null means the planet's resident field; base: also give xyz (Float32Array(M * 3)) at that base; lonlat: also give lonlat
// (Float64Array(M * 2), radians).  -> { source, info, sides, ring_start, ring_class, ring_of_side[, xyz][, lonlat] }
export function buildOutlineOnPlanet(planet, triangles, halfedges, source, opts) {
    const o = opts || {};
    const sid = typeof source === 'number' ? source : OUTLINE_SOURCES.indexOf(source);
    if (sid < 0 || sid >= OUTLINE_SOURCES.length) throw new RangeError(`buildOutline: unknown outline source '${source}' (one of ${OUTLINE_SOURCES.join(', ')})`);
    if (o.values !== undefined && o.values !== null && !(o.values instanceof Int32Array)) throw new TypeError('buildOutline: values must be an Int32Array of numRegions entries');
    const levels = o.levels === undefined || o.levels === null ? null : Float32Array.from(o.levels);
    const e = o.r_elevation || null;
    const only = o.onlyClass === undefined || o.onlyClass === null ? -1 : o.onlyClass;
    const info = addon.outlineBuild(planet, triangles, halfedges, sid, sid === 0 || sid === 3 ? e : null, o.values || null, levels, only);
    const M = info.boundarySides, R = info.rings;
    const res = { source: OUTLINE_SOURCES[sid], info };
    [M, R + 1, R, M].forEach((count, i) => { res[OUTLINE_FIELDS[i]] = addon.outlineDownload(planet, OUTLINE_FIELDS[i], count); });
    if (o.base !== undefined && o.base !== null) res.xyz = addon.outlinePositions(planet, M, o.base, e);
    if (o.lonlat) res.lonlat = addon.outlineLonLat(planet, M);
    return res;
}
// buildOutline(mesh, r_xyz, source, { r_elevation, values, levels, onlyClass, base, lonlat })
export function buildOutline(mesh, r_xyz, source, opts) { return buildOutlineOnPlanet(planetFor(mesh, r_xyz), mesh.triangles, mesh.halfedges, source, opts); }

// one object per ring, views into the result's arrays: { ring, class, sides[, xyz][, lonlat] }
export function outlineRings(result) {
    const start = result.ring_start, out = [];
    for (let r = 0; r + 1 < start.length; ++r) {
        const a = start[r], b = start[r + 1];
        const ring = { ring: r, class: result.ring_class[r], sides: result.sides.subarray(a, b) };
        if (result.xyz) ring.xyz = result.xyz.subarray(3 * a, 3 * b);
        if (result.lonlat) ring.lonlat = result.lonlat.subarray(2 * a, 2 * b);
        out.push(ring);
    }
    return out;
}

// A closed ring of longitudes (radians) cut where two consecutive vertices differ by more than pi: arrays of indices into the ring, one
// per piece.  An uncut ring gives one piece that ends with its first vertex again; a cut one gives its pieces in ring order, the one
// that holds vertex 0 last.
export function ringPieces(lon) {
    const n = lon.length;
    if (n === 0) return [];
    const cut = [];
    for (let i = 0; i < n; ++i) if (Math.abs(lon[i] - lon[(i + 1) % n]) > Math.PI) cut.push(i);
    if (cut.length === 0) { const all = Array.from({ length: n }, (_, i) => i); all.push(0); return [all]; }
    return cut.map((a, j) => {
        const first = a + 1;
        let last = cut[(j + 1) % cut.length];
        if (last < first) last += n;
        const piece = [];
        for (let i = first; i <= last; ++i) piece.push(i % n);
        return piece;
    });
}

// the rings as line segments, six floats each, every vertex joined to the next of its ring: what a LINES primitive draws
export function outlineSegments(result) {
    const xyz = result.xyz, start = result.ring_start;
    if (!(xyz instanceof Float32Array)) throw new TypeError("outlineSegments needs the result's xyz (buildOutline with base)");
    const out = new Float32Array(xyz.length * 2);
    for (let r = 0; r + 1 < start.length; ++r) {
        for (let k = start[r]; k < start[r + 1]; ++k) {
            const next = k + 1 < start[r + 1] ? k + 1 : start[r];
            for (let c = 0; c < 3; ++c) { out[6 * k + c] = xyz[3 * k + c]; out[6 * k + 3 + c] = xyz[3 * next + c]; }
        }
    }
    return out;
}

const degrees = (x) => x * 180 / Math.PI;

// A FeatureCollection with one feature per ring, in degrees (longitude, latitude): a closed LineString; for a ring that crosses the
// map's edge the pieces between its cuts (a LineString for one, a MultiLineString for more), so that nothing streaks across the
// map.  Properties: ring, class, and the entries of `properties`.
export function outlineToGeoJSON(result, properties) {
    if (!result.lonlat) throw new TypeError("outlineToGeoJSON needs the result's lonlat (buildOutline with lonlat)");
    const features = outlineRings(result).map((ring) => {
        const ll = ring.lonlat, lon = new Float64Array(ll.length / 2);
        for (let i = 0; i < lon.length; ++i) lon[i] = ll[2 * i];
        const lines = ringPieces(lon).map((idx) => (idx.length === 1 ? [idx[0], idx[0]] : idx).map((i) => [degrees(ll[2 * i]), degrees(ll[2 * i + 1])]));
        const geometry = lines.length === 1 ? { type: 'LineString', coordinates: lines[0] } : { type: 'MultiLineString', coordinates: lines };
        return { type: 'Feature', properties: Object.assign({ ring: ring.ring, class: ring.class }, properties || {}), geometry };
    });
    return JSON.stringify({ type: 'FeatureCollection', features });
}

// (x, y, shifted longitude) of vertices in the pixel frame of exportMap at width x width / 2, row 0 north, the centre meridian at centerLon
export function mapPixels(lonlat, width, centerLon) {
    const n = lonlat.length / 2, x = new Float64Array(n), y = new Float64Array(n), lon = new Float64Array(n);
    for (let i = 0; i < n; ++i) {
        let l = lonlat[2 * i] - (centerLon || 0);
        l = l > Math.PI ? l - 2 * Math.PI : (l < -Math.PI ? l + 2 * Math.PI : l);
        lon[i] = l;
        x[i] = (l / Math.PI + 1.0) * 0.5 * width;
        y[i] = (1.0 - lonlat[2 * i + 1] / (Math.PI / 2)) * 0.5 * Math.floor(width / 2);
    }
    return { x, y, lon };
}

// An SVG of width x width / 2 in the pixel frame of exportMap: one path per ring with its class and ring number as data attributes,
// cut like outlineToGeoJSON's, in the frame shifted to centerLon.
export function outlineToSvg(result, width, centerLon) {
    if (!result.lonlat) throw new TypeError("outlineToSvg needs the result's lonlat (buildOutline with lonlat)");
    if (!Number.isInteger(width) || width < 2 || width % 2) throw new RangeError(`outlineToSvg: width is ${width}, it must be even and at least 2`);
    const out = [`<svg xmlns="http://www.w3.org/2000/svg" width="${width}" height="${width / 2}" viewBox="0 0 ${width} ${width / 2}" fill="none" stroke="black" stroke-width="1">`];
    for (const ring of outlineRings(result)) {
        const { x, y, lon } = mapPixels(ring.lonlat, width, centerLon || 0);
        const d = ringPieces(lon).map((idx) => {
            const closed = idx.length > 1 && idx[0] === idx[idx.length - 1];      // the one piece of an uncut ring
            const pts = closed ? idx.slice(0, -1) : idx;
            return 'M' + pts.map((i) => `${x[i].toFixed(3)} ${y[i].toFixed(3)}`).join('L') + (closed ? 'Z' : '');
        });
        out.push(`<path data-ring="${ring.ring}" data-class="${ring.class}" d="${d.join(' ')}"/>`);
    }
    out.push('</svg>');
    return out.join('\n');
}
